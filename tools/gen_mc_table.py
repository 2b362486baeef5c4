#!/usr/bin/env python3
"""The 256-case marching-cubes table of 3dgp_amd/csrc/geometry.hip, derived rather than typed in.

Conventions (shared with geometry.hip and the tests):
  corner k = 4*dd + 2*dh + dw sits at offset (dd, dh, dw) of the cell's lower grid point, axis order (d, h, w) as the volume is indexed;
  bit k of the case is set when the corner's value is >= the threshold ("inside");
  edge e = 4*axis + 2*xb + xc runs along `axis` from the corner whose two other coordinates (in ascending axis order) are (xb, xc).

Derivation.  On every face of the cube the iso-line is fixed by the four corner signs of that face ALONE: each maximal run of inside corners
(walking the face's boundary) is cut off by one segment between the two sign-changing edges next to it; on the ambiguous face (inside
corners on one diagonal) that makes two segments, one around each inside corner.  Because the rule sees nothing but the face, the two cells
sharing a face draw the same segments on it -- the mesh cannot crack there, whatever the two cases are.  Segments are directed so that,
seen from outside the cube, the inside corners lie to their right; chained over the six faces they close into loops, and each loop is
triangulated.  With vertices in (d, h, w) read as a right-handed (x, y, z), every triangle's normal then points toward LOWER values.
A triangulation never uses a diagonal between two edges of one face (such a diagonal lies in the face, where the neighbour cell may draw
the same one: an edge with four triangles); among the admissible triangulations the one of least total diagonal length (edge midpoints) is
taken, ties by enumeration order, so the output is deterministic.

`python tools/gen_mc_table.py` rewrites 3dgp_amd/csrc/mc_table.inc; `--check` only compares.  tests/test_geometry.py imports `table()`,
`render_inc()` and `check_table()`.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC_PATH = os.path.join(REPO, '3dgp_amd', 'csrc', 'mc_table.inc')
MAX_TRIS = 5            # widest row the kernels reserve; the derivation asserts it


def corner_offset(k):
    return ((k >> 2) & 1, (k >> 1) & 1, k & 1)


def corner_index(p):
    return 4 * p[0] + 2 * p[1] + p[2]


def edge_info(e):
    """-> (axis, offset (dd, dh, dw) of the edge's lower corner)."""
    axis, xb, xc = e >> 2, (e >> 1) & 1, e & 1
    b, c = [a for a in range(3) if a != axis]
    off = [0, 0, 0]
    off[b], off[c] = xb, xc
    return axis, tuple(off)


def edge_corners(e):
    axis, off = edge_info(e)
    hi = list(off)
    hi[axis] = 1
    return corner_index(off), corner_index(hi)


def edge_between(k0, k1):
    for e in range(12):
        if set(edge_corners(e)) == {k0, k1}:
            return e
    raise ValueError((k0, k1))


def edge_midpoint(e):
    axis, off = edge_info(e)
    m = [float(x) for x in off]
    m[axis] = 0.5
    return m


def edge_faces(e):
    """The two faces (axis, side) an edge lies on."""
    axis, off = edge_info(e)
    return {(a, off[a]) for a in range(3) if a != axis}


def face_corners(a, side):
    """The four corners of face (axis a, side), counter-clockwise seen from outside the cube."""
    u, v = ((a + 1) % 3, (a + 2) % 3) if side == 1 else ((a + 2) % 3, (a + 1) % 3)       # u x v = outward normal
    out = []
    for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):
        p = [0, 0, 0]
        p[a], p[u], p[v] = side, cu, cv
        out.append(corner_index(p))
    return out


FACES = [(a, s) for a in range(3) for s in (0, 1)]


def face_segments(case, a, side):
    """Directed segments (edge_from, edge_to) the iso-surface leaves on one face: a function of that face's four corner signs only."""
    cs = face_corners(a, side)
    s = [(case >> k) & 1 for k in cs]
    if sum(s) in (0, 4):
        return []
    segs = []
    for i in range(4):
        if s[i] and not s[i - 1]:                       # a run of inside corners starts at i
            j = i
            while s[(j + 1) % 4]:
                j += 1
            e_in = edge_between(cs[i - 1], cs[i])       # the edge before the run
            e_out = edge_between(cs[j % 4], cs[(j + 1) % 4])        # the edge after it
            segs.append((e_in, e_out))
    return segs


def loops_of(case):
    nxt = {}
    for a, s in FACES:
        for e0, e1 in face_segments(case, a, s):
            assert e0 not in nxt, (case, e0)
            nxt[e0] = e1
    crossing = {e for e in range(12) if ((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1}
    assert set(nxt) == crossing and set(nxt.values()) == crossing, case
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        loops.append(loop)
    return loops


def _triangulations(idx):
    """Every triangulation of the polygon idx[0..n-1] as lists of index triples (orientation kept)."""
    n = len(idx)
    if n < 3:
        yield []
        return
    if n == 3:
        yield [tuple(idx)]
        return
    for k in range(1, n - 1):                           # the triangle on the side idx[0]-idx[-1]
        for left in _triangulations(idx[:k + 1]):
            for right in _triangulations(idx[k:]):
                yield left + [(idx[0], idx[k], idx[-1])] + right


def _dist(e0, e1):
    return sum((x - y) ** 2 for x, y in zip(edge_midpoint(e0), edge_midpoint(e1))) ** 0.5


def triangulate(loop):
    sides = {frozenset((loop[i], loop[(i + 1) % len(loop)])) for i in range(len(loop))}
    best = None
    for tris in _triangulations(list(loop)):
        diags = {frozenset(p) for t in tris for p in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))} - sides
        if any(edge_faces(min(d)) & edge_faces(max(d)) for d in diags):
            continue
        cost = round(sum(_dist(*sorted(d)) for d in diags), 9)
        if best is None or cost < best[0]:
            best = (cost, tris)
    assert best is not None, f'no admissible triangulation of loop {loop}'
    return [(t[0], t[1], t[2]) for t in best[1]]


_TABLE = None


def table():
    """-> list of 256 lists of triangles, each a triple of edge ids."""
    global _TABLE
    if _TABLE is None:
        out = []
        for case in range(256):
            tris = [t for loop in loops_of(case) for t in triangulate(loop)]
            assert len(tris) <= MAX_TRIS, (case, len(tris))
            out.append(tris)
        _TABLE = out
    return _TABLE


def check_table(tab):
    """Raises AssertionError unless `tab` is a closed, consistently oriented, face-consistent 256-case table."""
    assert len(tab) == 256
    for case, tris in enumerate(tab):
        crossing = {e for e in range(12) if ((case >> edge_corners(e)[0]) ^ (case >> edge_corners(e)[1])) & 1}
        assert {e for t in tris for e in t} == crossing, case
        directed = [p for t in tris for p in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))]
        assert len(set(directed)) == len(directed), case
        on_face = {}
        for p in directed:
            common = edge_faces(p[0]) & edge_faces(p[1])
            if common:
                assert len(common) == 1
                on_face.setdefault(next(iter(common)), []).append(p)
            else:                                       # an interior edge: its reverse closes it inside the cell
                assert (p[1], p[0]) in directed, (case, p)
        for a, s in FACES:
            assert sorted(on_face.get((a, s), [])) == sorted(face_segments(case, a, s)), (case, a, s)
        for t in tris:                                  # normal toward lower values: away from the inside corners' side
            p = [edge_midpoint(e) for e in t]
            u = [p[1][i] - p[0][i] for i in range(3)]
            v = [p[2][i] - p[0][i] for i in range(3)]
            n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
            assert any(abs(x) > 1e-12 for x in n), (case, t)
    # single-corner cases pin the orientation convention itself
    for k in range(8):
        (t,) = tab[1 << k]
        p = [edge_midpoint(e) for e in t]
        u = [p[1][i] - p[0][i] for i in range(3)]
        v = [p[2][i] - p[0][i] for i in range(3)]
        n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
        c = corner_offset(k)
        centre = [sum(q[i] for q in p) / 3 for i in range(3)]
        assert sum(n[i] * (centre[i] - c[i]) for i in range(3)) > 0, k       # away from the inside corner


def render_inc(tab=None):
    tab = table() if tab is None else tab
    lines = ['// mc_table.inc -- GENERATED by tools/gen_mc_table.py; do not edit (tests/test_geometry.py compares it with the generator).',
             '// Corner k = 4*dd + 2*dh + dw, case bit k = (value >= threshold), edge e = 4*axis + 2*xb + xc (see the generator).',
             '// Row: number of triangles, then 3 edge ids per triangle (normal toward lower values), padded with 0 to 15.',
             '// MC_TABLE_QUAL: the including file\'s storage qualifiers (geometry.hip: __device__ const).',
             f'#define MC_MAX_TRIS {MAX_TRIS}',
             '#ifndef MC_TABLE_QUAL',
             '#define MC_TABLE_QUAL static const',
             '#endif',
             'MC_TABLE_QUAL unsigned char MC_TABLE[256][16] = {']
    for case, tris in enumerate(tab):
        row = [len(tris)] + [e for t in tris for e in t]
        row += [0] * (16 - len(row))
        lines.append('    {' + ', '.join(f'{x:2d}' for x in row) + '},' + f'   // {case:3d}')
    lines.append('};')
    return '\n'.join(lines) + '\n'


def main(argv):
    tab = table()
    check_table(tab)
    text = render_inc(tab)
    if '--check' in argv:
        same = os.path.exists(INC_PATH) and open(INC_PATH).read() == text
        print('mc_table.inc', 'matches' if same else 'DIFFERS from', 'the generator')
        return 0 if same else 1
    with open(INC_PATH, 'w') as f:
        f.write(text)
    hist = [sum(1 for t in tab if len(t) == n) for n in range(MAX_TRIS + 1)]
    print(f'wrote {INC_PATH}: cases by triangle count {hist}')
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
