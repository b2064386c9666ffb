"""A small zoo of hand-made scenes for the lean wavefront's secondary-ray paths
(miss cull, direct lists, direct resolve, clip walk), whose occluder boxes differ
from scene01's, kquads' and seam's: lists of one triangle, many unlisted boxes
with gaps and overlaps between them, listed boxes of glass and mirror, boxes
the clustering merged at a cost.

* single   the floor fan, one red triangle and one emitting triangle (the only
           lists, one triangle each) and a back wall built as a fan of three (unlisted)
* tetras   the floor fan, five tetrahedra (red, mirror, glass, grey, red): three in a
           row along the view axis, two whose boxes overlap; only the quad light is listed
* panes    the floor fan, a red back wall, a glass pane, a mirror pane and the quad light:
           four listed boxes, two of them specular
* many     the floor fan, twelve small quads scattered over the scene (materials cycling
           red / grey / mirror / glass) and the quad light: more objects than boxes, so the
           clustering merges some of them around empty space

All text is built from the literal coordinates below by Python float arithmetic and
%.6f, the same on every machine; nothing is random at test time.  `zoo_scenes` is
a session fixture, imported by the modules that use it (as dl_scenes is).
"""
import math

import pytest

MTL = ("newmtl grey\nKd 0.7 0.7 0.7\nKa 0 0 0\nnewmtl red\nKd 0.7 0.3 0.3\nKa 0 0 0\n"
       "newmtl glow\nKd 0.5 0.5 0.5\nKa 0.6 0.5 0.4\n"
       "newmtl mirror\nKd 0 0 0\nKa 0 0 0\nKs 1 1 1\nNs 1000\n"
       "newmtl glass\nKd 0.5 0.5 0.5\nKa 0 0 0\nTr 0.9\nNi 1.5\n")

ZOO = ("single", "tetras", "panes", "many")
ZOO_CAM = dict(eye=(0.0, 5.0, 7.0), direction=(0.0, -0.3, -1.0))

FAN = [(-6, 0, -6), (6, 0, -6), (6, 0, 6), (0, 0, 6), (-6, 0, 6)]            # kquads' floor: 3 triangles
LIGHT = [(-2, 8, -4), (2, 8, -4), (2, 8, 0), (-2, 8, 0)]                     # kquads' light, facing down
BACK_FAN = [(-6, 0, -6), (6, 0, -6), (6, 8, -6), (0, 8, -6), (-6, 8, -6)]    # a wall of 3 triangles
BACK_QUAD = [(-6, 0, -6), (6, 0, -6), (6, 8, -6), (-6, 8, -6)]

SINGLE_RED = [(-3, 1, -3), (3, 1, -4), (0, 5, -5)]
SINGLE_GLOW = [(-2, 8, -4), (2, 8, -4), (0, 8, 0)]
# from the height of the lone red triangle's base, a little in front of it, looking up its face:
# 89% of a 64 x 64 frame's pixel centres see it
SINGLE_CAM_BELOW = dict(eye=(0.0, 1.0, -2.6), direction=(0.0, 0.6, -1.0))

TETRA = [(1, 0, -.7), (-1, 0, -.7), (0, 1, .7), (0, -1, .7)]
TETRAS = [((0, 1.2, 2), 1.0, "red"), ((0, 2, -1), 1.4, "mirror"), ((0, 1.5, -4.5), 1.2, "glass"),
          ((-3.5, 1.5, 0), 1.3, "grey"), ((-2.4, 2.2, -0.8), 1.0, "red")]
TETRAS_MIDDLE = 1                                                            # (the eye-inside case's tetrahedron)

GLASS_PANE = [(-4, 0, -1), (0, 0, -2), (0, 5, -2), (-4, 5, -1)]
MIRROR_PANE = [(1, 0, -3), (5, 0, 0), (5, 5, 0), (1, 5, -3)]

# twelve quads: centre, half side U, half side V (scattered once by hand and by dice: half sides
# 0.5..1.5, centres in (-5..5, 0.5..6, -5..3); 3 decimals); corners c -+ U -+ V.  Three groups of
# three lie close enough for the clustering to merge each into one thick box of six triangles;
# three larger quads stand alone and keep their lists (a grey, a mirror and a glass one)
MANY = [
    ((-4.2, 1.5, -4.1), (0.713, 0.402, -0.331), (-0.298, 0.911, 0.465)),          # left, back, low: 0, 5, 10
    ((2.871, 4.655, -1.904), (1.305, -0.212, 0.452), (0.254, 1.402, -0.076)),     # on its own
    ((3.6, 2.3, -4.2), (-0.433, 0.250, 0.000), (0.392, 0.679, 0.991)),            # right, back, low: 2, 3, 9
    ((4.1, 1.1, -3.4), (0.000, 0.611, 0.611), (1.210, 0.000, 0.000)),
    ((-4.4, 4.9, 1.2), (0.355, 0.355, -0.870), (0.581, -0.581, 0.000)),           # left, front, high: 4, 8, 11
    ((-3.0, 0.9, -4.4), (0.950, 0.000, 0.312), (-0.180, 0.733, 0.548)),
    ((-0.6, 2.0, 1.8), (1.112, 0.354, 0.607), (-0.354, 1.212, 0.000)),            # on its own
    ((3.342, 3.016, 2.210), (-0.55, 0.433, 1.166), (1.05, 0.775, 0.000)),         # on its own
    ((-3.7, 3.8, 2.5), (0.489, 0.104, 0.000), (-0.208, 0.978, 0.978)),
    ((2.9, 3.2, -4.6), (0.862, 0.000, -0.498), (0.249, 0.748, 0.431)),
    ((-4.6, 2.7, -3.4), (0.000, 1.100, 0.000), (0.389, 0.000, 0.389)),
    ((-4.5, 5.6, 2.4), (0.741, 0.296, 0.000), (0.000, 0.000, 1.313)),
]
MANY_MATERIALS = ("red", "grey", "mirror", "glass")


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _normal(p, towards=None):
    """the unit normal of the polygon's first three corners, turned towards a direction if one is given"""
    n = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
    ln = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    n = (n[0] / ln, n[1] / ln, n[2] / ln)
    if towards is not None and n[0] * towards[0] + n[1] * towards[1] + n[2] * towards[2] < 0:
        n = (-n[0], -n[1], -n[2])
    return n


class _Obj:
    """OBJ text, one group per polygon or fan; a polygon is one face line, a fan one triangle per line"""

    def __init__(self, name):
        self.v, self.vn, self.f = ["mtllib %s.mtl" % name], [], []
        self.nv = self.nn = 0

    def _add(self, group, material, corners, normal):
        self.v += ["v %.6f %.6f %.6f" % tuple(float(x) for x in c) for c in corners]
        self.vn.append("vn %.6f %.6f %.6f" % tuple(float(x) + 0.0 for x in normal))       # (+ 0.0: no "-0")
        self.nn += 1
        self.f += ["g " + group, "usemtl " + material]
        ids = ["%d//%d" % (self.nv + 1 + i, self.nn) for i in range(len(corners))]
        self.nv += len(corners)
        return ids

    def polygon(self, group, material, corners, towards=None):
        self.f.append("f " + " ".join(self._add(group, material, corners, _normal(corners, towards))))

    def fan(self, group, material, corners, towards=None):
        ids = self._add(group, material, corners, _normal(corners, towards))
        self.f += ["f %s %s %s" % (ids[0], ids[i], ids[i + 1]) for i in range(1, len(ids) - 1)]

    def text(self):
        return "\n".join(self.v + self.vn + self.f) + "\n"


def _base(name):
    o = _Obj(name)
    o.fan("floor", "grey", FAN, towards=(0, 1, 0))
    return o


def tetra_corners(centre, radius):
    return [tuple(centre[a] + radius * t[a] for a in range(3)) for t in TETRA]


def many_corners(q):
    c, u, v = q
    return [tuple(c[a] + su * u[a] + sv * v[a] for a in range(3)) for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def single_obj():
    o = _base("single")
    o.polygon("tri", "red", SINGLE_RED, towards=(0, 0, 1))
    o.polygon("lamp", "glow", SINGLE_GLOW, towards=(0, -1, 0))
    o.fan("back", "grey", BACK_FAN, towards=(0, 0, 1))
    return o.text()


def tetras_obj():
    o = _base("tetras")
    for i, (c, r, mat) in enumerate(TETRAS):
        p = tetra_corners(c, r)
        for j, face in enumerate(((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))):
            tri = [p[k] for k in face]
            out = _sub(tuple(sum(t[a] for t in tri) / 3.0 for a in range(3)), c)          # away from the centre
            o.polygon("tetra%d_%d" % (i, j), mat, tri, towards=out)
    o.polygon("light", "glow", LIGHT, towards=(0, -1, 0))
    return o.text()


def panes_obj():
    o = _base("panes")
    o.polygon("wall", "red", BACK_QUAD, towards=(0, 0, 1))
    o.polygon("glass", "glass", GLASS_PANE, towards=(0, 0, 1))
    o.polygon("mirror", "mirror", MIRROR_PANE, towards=(0, 0, 1))
    o.polygon("light", "glow", LIGHT, towards=(0, -1, 0))
    return o.text()


def many_obj():
    o = _base("many")
    for i, q in enumerate(MANY):
        o.polygon("quad%02d" % i, MANY_MATERIALS[i % 4], many_corners(q), towards=(0, 0.3, 1))
    o.polygon("light", "glow", LIGHT, towards=(0, -1, 0))
    return o.text()


OBJS = {"single": single_obj, "tetras": tetras_obj, "panes": panes_obj, "many": many_obj}


@pytest.fixture(scope="session")
def zoo_scenes(tmp_path_factory):
    """name -> .obj path"""
    paths = {}
    for name in ZOO:
        d = tmp_path_factory.mktemp("zoo_" + name)
        (d / (name + ".obj")).write_text(OBJS[name]())
        (d / (name + ".mtl")).write_text(MTL)
        paths[name] = str(d / (name + ".obj"))
    return paths


def tri_groups(model, scene):
    """kd id -> index of the OBJ group its triangle is in"""
    import numpy as np
    of = np.full(model.info()["n_triangles"], -1, np.int64)
    for i, (_, tris) in enumerate(sorted(model.groups().items())):
        of[tris] = i
    return of[scene.kd()[2]]
