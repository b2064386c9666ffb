"""Exact-arithmetic classifier of brute-force / KD-walk disagreements, shared by
tests/test_brute_pins.py and tests/test_ray_contract_cpu.py: the Cramer test
of CUTracer.cu:58-92 in rational arithmetic on the float inputs."""
from fractions import Fraction as F


def exact_cramer(kv, tri, o, d):
    """CUTracer.cu:58-92's beta, gamma, t in exact rational arithmetic (float inputs)."""
    a, b, c = ([F(float(x)) for x in v] for v in kv[tri])
    oo = [F(float(x)) for x in o]
    dd = [F(float(x)) for x in d]

    def det(m):
        return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    col = lambda u, v, w: [u[0], v[0], w[0], u[1], v[1], w[1], u[2], v[2], w[2]]  # noqa: E731
    ab = [a[i] - b[i] for i in range(3)]
    ac = [a[i] - c[i] for i in range(3)]
    ao = [a[i] - oo[i] for i in range(3)]
    dA = det(col(ab, ac, dd))
    if dA == 0:
        return None
    return det(col(ao, ac, dd)) / dA, det(col(ab, ao, dd)) / dA, det(col(ab, ac, ao)) / dA


def float_artifact(kv, o, d, tb, hb, tk, hk, origin_shortcut=True):
    """A brute-force / KD disagreement that exact arithmetic resolves: the float
    Cramer test accepted a triangle that the exact test rejects, the two hits'
    float t order differs from their exact order, or (origin_shortcut, rays of
    unit direction only: t is a distance there) the hit touches the origin
    (t < 1e-5: the origin lies on a triangle edge)."""
    if origin_shortcut and ((tb >= 0 and hb[2] < 1e-5) or (tk >= 0 and hk[2] < 1e-5)):
        return True
    ex = {}
    for t in {int(tb), int(tk)} - {-1}:
        e = exact_cramer(kv, t, o, d)
        if e is None or not (e[0] > 0 and e[1] > 0 and e[0] + e[1] < 1 and e[2] > 0):
            return True            # the float test accepted an exact miss
        ex[t] = e[2]
    if tb >= 0 and tk >= 0:
        return ex[int(tb)] >= ex[int(tk)]   # exact order disagrees with the float order
    return False
