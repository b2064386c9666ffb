"""Scenes at the ends of the material space, built from tests/_zoo.py's geometry:
every other parity scene renders `Tr 0.9, Ni 1.5` glass, integer `Ns` in
{5 .. 1000}, `Ks` 1 or 0.5, `Kd` <= 1 and plain diffuse emitters.

* edges     the floor fan, the red back wall, the quad light, `many`'s twelve quads and
            `tetras`' five tetrahedra, their materials cycling through EDGE_MATERIALS:
            the class boundaries of scatter / material_class (Ns exactly 1 with a Ks
            line: diffuse; Ns 1.5: Phong with Ns_u = 1; a Ks line without Ns: the
            loader's Ns = 2), Phong exponents that are no integer, huge, or beyond the
            unsigned range (Ns 5e9: Ns_u clamps to 0xFFFFFF00), Fresnel ends (Ni 1, 3
            and 0.8; Tr 1, 2 -- a probability above 1 -- and 0.001), coloured Ks, a Kd
            above 1, and an emitter that is also glass (is_emitter wins)
* nanfloor  `panes` with the floor made `Tr 0.9, Ni 0.8`: entering refraction beyond the
            critical angle takes the square root of a negative number, as the reference
            does, so the renderer itself makes all-NaN rays (direction, then origin
            hit + 0.01 * direction) that go through every cull, list and walk
* gain20    `panes` with `Kd 1e20 ..` on the floor and the wall: the throughput overflows
            to inf after two bounces and the terminal query's `inf * 0` is NaN -- where
            the terminal cull would store 0.  The cull's admission rule (plan.cpp:
            log2(max(1, cull_gain)) * max_depth < 127) must turn it off
* gain18 / gain19   the same with Kd 2^18 and 2^19: either side of that rule at depth 7
            (18 * 7 = 126 < 127 <= 133 = 19 * 7); both images are finite

All text is built from _zoo's literal coordinates, nothing is random.  Every scene has
fewer than 60 triangles (in LDS under layout="auto").  `matzoo_scenes` is a session
fixture, imported by the modules that use it (as zoo_scenes is).
"""
import pytest

from _zoo import (BACK_QUAD, LIGHT, MANY, MTL, TETRAS, _base, _sub, many_corners, panes_obj, tetra_corners)

MATZOO = ("edges", "nanfloor", "gain20", "gain18", "gain19")
GAIN_KD = {"gain20": "1e20", "gain18": "262144", "gain19": "524288"}

# name -> .mtl lines.  (A Ks line sets Ns = 2 in the reference's loader, so Ns comes after Ks.)
EDGE_MATERIALS = (
    ("ns1", "Kd 0.6 0.6 0.2\nKs 1 1 1\nNs 1"),                   # exactly 1: diffuse (Ns > 1 is Phong)
    ("ns1_5", "Kd 0.1 0.1 0.1\nKs 0.9 0.9 0.9\nNs 1.5"),         # Phong; CV: (unsigned)1.5 + 1, QE: 2.5
    ("ns_default", "Kd 0.1 0.1 0.1\nKs 0.8 0.8 0.8"),            # the loader's Ns = 2
    ("ns2_7", "Kd 0.1 0.1 0.1\nKs 0.9 0.9 0.9\nNs 2.7"),
    ("ns1e6", "Kd 0 0 0\nKs 1 1 1\nNs 1e6"),
    ("ns5e9", "Kd 0 0 0\nKs 1 1 1\nNs 5e9"),                     # above 2^32: Ns_u = 0xFFFFFF00
    ("ni1", "Kd 0.5 0.5 0.5\nTr 0.9\nNi 1"),
    ("ni3", "Kd 0.5 0.5 0.5\nTr 0.9\nNi 3"),
    ("ni0_8", "Kd 0.5 0.5 0.5\nTr 0.9\nNi 0.8"),                 # NaN beyond the critical angle
    ("tr1", "Kd 0.5 0.5 0.5\nTr 1\nNi 1.5"),
    ("tr2", "Kd 0.5 0.5 0.5\nTr 2\nNi 1.5"),                     # Tr * F can exceed every uniform
    ("tr0_001", "Kd 0.5 0.5 0.5\nTr 0.001\nNi 1.5"),
    ("ks_rgb", "Kd 0.2 0.2 0.2\nKs 0.9 0.5 0.2\nNs 20"),
    ("kd2", "Kd 2 0.5 0"),
    ("glowglass", "Kd 0.5 0.5 0.5\nKa 0.3 0.4 0.5\nTr 0.9\nNi 1.5"),   # emits: never scatters
)


def _mtl(extra):
    """_zoo's materials and `extra`'s, each with a Ka line (0 0 0 unless it has its own)"""
    return MTL + "".join("newmtl %s\n%s\n%s" % (n, t, "" if "Ka " in t else "Ka 0 0 0\n") for n, t in extra)


def same_nan_aware(a, b):
    """bits equal wherever neither side is NaN, and NaN in exactly the same places (a NaN's sign
    and payload are not the renderer's to define)"""
    import numpy as np
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _replace_kd(mtl, material, kd):
    """the .mtl text with `material`'s Kd line replaced, other lines kept"""
    out, cur, done = [], None, False
    for line in mtl.splitlines():
        if line.startswith("newmtl"):
            cur = line.split()[1]
        if cur == material and line.startswith("Kd "):
            line, done = kd, True
        out.append(line)
    assert done, material
    return "\n".join(out) + "\n"


def edge_material_of():
    """OBJ group -> material name of the edges scene's 17 objects"""
    names = [n for n, _ in EDGE_MATERIALS]
    of = {"quad%02d" % i: names[i % len(names)] for i in range(len(MANY))}
    of.update({"tetra%d" % j: names[(len(MANY) + j) % len(names)] for j in range(len(TETRAS))})
    return of


def edges_obj():
    o = _base("edges")
    of = edge_material_of()
    o.polygon("wall", "red", BACK_QUAD, towards=(0, 0, 1))
    for i, q in enumerate(MANY):
        o.polygon("quad%02d" % i, of["quad%02d" % i], many_corners(q), towards=(0, 0.3, 1))
    for j, (c, r, _) in enumerate(TETRAS):
        p = tetra_corners(c, r)
        for k, face in enumerate(((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))):
            tri = [p[v] for v in face]
            out = _sub(tuple(sum(t[a] for t in tri) / 3.0 for a in range(3)), c)          # away from the centre
            o.polygon("tetra%d_%d" % (j, k), of["tetra%d" % j], tri, towards=out)
    o.polygon("light", "glow", LIGHT, towards=(0, -1, 0))
    return o.text()


def edges_mtl(**override):
    """the edges scene's .mtl text, with the lines of the named materials replaced"""
    assert set(override) <= {n for n, _ in EDGE_MATERIALS}
    return _mtl(tuple((n, override.get(n, t)) for n, t in EDGE_MATERIALS))


def scene_text(name):
    """(file stem, .obj text, .mtl text)"""
    if name == "edges":
        return "edges", edges_obj(), edges_mtl()
    if name == "nanfloor":                                         # (`grey` is the floor's alone in panes)
        grey = "newmtl grey\nKd 0.7 0.7 0.7\n"
        assert grey in MTL
        return "panes", panes_obj(), MTL.replace(grey, grey + "Tr 0.9\nNi 0.8\n")
    kd = GAIN_KD[name[:6]]
    mtl = _replace_kd(_replace_kd(MTL, "grey", "Kd %s 0.7 0.7" % kd), "red", "Kd %s 0.3 0.3" % kd)
    if name.endswith("_nocull"):                                   # a negative Ka on a non-emitter: no emitter boxes
        mirror = "newmtl mirror\nKd 0 0 0\nKa 0 0 0\n"
        assert mirror in mtl
        mtl = mtl.replace(mirror, "newmtl mirror\nKd 0 0 0\nKa -0.5 0 0\n")
    return "panes", panes_obj(), mtl


# gain19 with a non-emitter of negative Ka: the host makes no emitter boxes for such a scene
# (tests/test_terminal_cull.py `negative`), so no render of it culls a terminal ray, and a
# negative Ka changes no ray: the counters of a render that culls nothing, for gain19's rays
TWINS = ("gain19_nocull",)


@pytest.fixture(scope="session")
def matzoo_scenes(tmp_path_factory):
    """name -> .obj path"""
    paths = {}
    for name in MATZOO + TWINS:
        stem, obj, mtl = scene_text(name)
        d = tmp_path_factory.mktemp("matzoo_" + name)
        (d / (stem + ".obj")).write_text(obj)
        (d / (stem + ".mtl")).write_text(mtl)
        paths[name] = str(d / (stem + ".obj"))
    return paths
