"""User-defined implicit surfaces that no built-in shape reproduces (a torus section, a saddle, an off-axis paraboloid
section) and implicit twins of built-in shapes (sphere cap, cylinder wall), built from `ns` so that the reference and this
package run the very same user code (surfaces.py:5-65: f / normal / within_boundary / get_bbox_local are the contract)."""
import numpy as np


def _unit(v):
    v = np.asarray(v, dtype=float)
    return v / np.linalg.norm(v)


def implicit_surface_classes(ns):
    class Torus(ns.Surface):
        """Section of the torus about the local z axis (tube radius r, centre-line radius R) around its outer equator,
        shifted so that the vertex is the local origin: a toroidal (astigmatic) mirror, x = 0 at the vertex, x < 0 inside."""

        def __init__(self, R, r, a):
            super().__init__()
            self.planar = False
            self.R, self.r, self.a = R, r, a

        def _q(self, P):
            X = P[0] + self.R + self.r
            return X, X * X + P[1] ** 2 + P[2] ** 2 + self.R**2 - self.r**2

        def f(self, P):
            X, s = self._q(P)
            return s * s - 4 * self.R**2 * (X * X + P[1] ** 2)

        def normal(self, P):
            X, s = self._q(P)
            g = np.array([4 * s * X - 8 * self.R**2 * X, 4 * s * P[1] - 8 * self.R**2 * P[1], 4 * s * P[2]])
            return _unit(g)

        def within_boundary(self, P):
            return P[1] ** 2 + P[2] ** 2 <= self.a**2

        def get_bbox_local(self):
            a = self.a
            sag = a * a / (self.R + self.r) + a * a / self.r
            return (-sag, 0.02 * a, -a, a, -a, a)

    class Saddle(ns.Surface):
        """x = -(y^2 - z^2) / (4 F): a saddle (not a surface of revolution), disc aperture."""

        def __init__(self, F, a):
            super().__init__()
            self.planar = False
            self.F, self.a = F, a

        def f(self, P):
            return P[0] + (P[1] ** 2 - P[2] ** 2) / (4 * self.F)

        def normal(self, P):
            return _unit([1.0, P[1] / (2 * self.F), -P[2] / (2 * self.F)])

        def within_boundary(self, P):
            return P[1] ** 2 + P[2] ** 2 <= self.a**2

        def get_bbox_local(self):
            s = self.a**2 / (4 * self.F)
            return (-s, s, -self.a, self.a, -self.a, self.a)

    class OffAxisParaboloid(ns.Surface):
        """The section of x = -(y^2 + z^2) / (4 F) centred at y = y0, with that point as the local origin; disc aperture."""

        def __init__(self, F, y0, a):
            super().__init__()
            self.planar = False
            self.F, self.y0, self.a = F, y0, a

        def f(self, P):
            return P[0] + ((P[1] + self.y0) ** 2 + P[2] ** 2 - self.y0**2) / (4 * self.F)

        def normal(self, P):
            return _unit([1.0, (P[1] + self.y0) / (2 * self.F), P[2] / (2 * self.F)])

        def within_boundary(self, P):
            return P[1] ** 2 + P[2] ** 2 <= self.a**2

        def get_bbox_local(self):
            a, y0, F = self.a, self.y0, self.F
            return (-(2 * a * abs(y0) + 2 * a * a) / (4 * F), 2 * a * abs(y0) / (4 * F), -a, a, -a, a)

    class ImplicitSphere(ns.Surface):
        """The reference's Sphere cap (surfaces.py:284-336: centre at the local origin, x in [R - h, R]) written as |P|^2 - R^2."""

        def __init__(self, radius, height):
            super().__init__()
            self.planar = False
            self.radius, self.height = radius, height

        def f(self, P):
            return P[0] ** 2 + P[1] ** 2 + P[2] ** 2 - self.radius**2

        def normal(self, P):
            return np.asarray(P, dtype=float) / self.radius

        def within_boundary(self, P):
            return self.radius - self.height - 1e-12 <= P[0] <= self.radius + 1e-12

        def get_bbox_local(self):
            h = np.sqrt(self.radius**2 - (self.radius - self.height) ** 2)
            return (self.radius - self.height, self.radius, -h, h, -h, h)

    class ImplicitCylinder(ns.Surface):
        """The reference's Cylinder wall about local z (surfaces.py:212-281, full turn) written as x^2 + y^2 - R^2."""

        def __init__(self, radius, height):
            super().__init__()
            self.planar = False
            self.radius, self.height = radius, height

        def f(self, P):
            return P[0] ** 2 + P[1] ** 2 - self.radius**2

        def normal(self, P):
            return np.array([P[0], P[1], 0.0]) / self.radius

        def within_boundary(self, P):
            return -self.height / 2 <= P[2] <= self.height / 2

        def get_bbox_local(self):
            r, h = self.radius, self.height / 2
            return (-r, r, -r, r, -h, h)

    class CurvedMirror(ns.BaseMirror):
        def __init__(self, origin, surface, **kwargs):
            super().__init__(origin, **kwargs)
            self.surface = surface

    class CurvedInterface(ns.BaseRefraciveSurface):
        def __init__(self, origin, surface, **kwargs):
            super().__init__(origin, **kwargs)
            self.surface = surface

    return dict(Torus=Torus, Saddle=Saddle, OffAxisParaboloid=OffAxisParaboloid, ImplicitSphere=ImplicitSphere,
                ImplicitCylinder=ImplicitCylinder, CurvedMirror=CurvedMirror, CurvedInterface=CurvedInterface)


W0 = 50e-4


def g29_implicit_surfaces(ns):
    """A saddle glass interface (front of a thick plate whose back is a built-in plane face), a partially reflecting toroidal
    mirror, a partially reflecting off-axis paraboloid section and a convex implicit sphere mirror, in a row along x.  Rays on
    axis, tilted, one that misses everything and one at the edge of the saddle's disc aperture."""
    U = implicit_surface_classes(ns)
    R = 20.0
    front = U["CurvedInterface"]([3, 0, 0], U["Saddle"](8.0, 1.5), n1=1.0, n2=1.5).RotZ(np.pi)
    back = ns.CircleRefractive([3.8, 0, 0], radius=1.5, n1=1.0, n2=1.5)
    torus = U["CurvedMirror"]([8, 0, 0], U["Torus"](10.0, 4.0, 1.5), reflectivity=0.3, transmission=0.7).RotZ(np.pi + 0.02)
    oap = U["CurvedMirror"]([12, 0, 0], U["OffAxisParaboloid"](6.0, 2.0, 1.5), reflectivity=0.5, transmission=0.5).RotZ(np.pi - 0.03)
    sphere = U["CurvedMirror"]([16 + R, 0, 0], U["ImplicitSphere"](R, 0.2)).RotZ(np.pi)
    rays = [ns.Ray([0, y, z], [1, dy, dz], wavelength=wl, w0=W0)
            for wl, y, z, dy, dz in ((633e-7, 0.0, 0.0, 0.0, 0.0), (633e-7, 0.3, 0.1, 0.0, 0.0), (633e-7, -0.45, -0.2, 0.01, 0.0),
                                     (450e-7, 0.2, 0.3, -0.02, 0.01), (850e-7, -0.1, -0.35, 0.015, -0.01), (633e-7, 0.0, 0.5, 0.0, 0.03),
                                     (633e-7, 3.0, 0.0, 0.0, 0.0), (633e-7, 1.4999, 0.0, 0.0, 0.0))]
    return dict(components=[front, back, torus, oap, sphere], monitors=[], rays=rays, limit={"max_trace_num": 40})


IMPLICIT_SCENES = {"g29_implicit_surfaces": g29_implicit_surfaces}
