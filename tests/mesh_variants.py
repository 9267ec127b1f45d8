"""Renumbered variants of a gmsh 2.2 ASCII mesh, and the topology cases a mesh reaches.

Everything that crosses an un_ele face branches on (face, fNeig, Dir): update_overlaps' slot
arithmetic, the oracle's overlap_kslot and fsx, the device halo tables, k_face_pp's ghost words, the
chain hand-offs and the exchange plans. An interior face can show 18 such triples -- face and fNeig
1..3, Dir 0/1 -- and which ones a mesh shows depends only on how its file numbers the nodes of each
triangle and orders the triangles (CheckNeig visits pairs in file order). `renumber` rewrites a
mesh with the same triangles numbered differently: the same geometry, other triples.

    renumber(src, dst, seed)      the variant file, deterministic in seed
    interface_triples(mesh)       {(face, fNeig, Dir)} over the interior faces (1-based faces)
    boundary_patterns(mesh)       {tuple of an un_ele's boundary faces}, () for an inner un_ele

`mesh` is oracle_lib.read_msh's (or pamg.Mesh's) object: flat Neig / fNeig / Dir of shape (3, U),
column-major. tests/meshes/*_rn.msh were written by this module (see VARIANTS).
"""
import os

import numpy as np

TRIANGLE = 2
# element types ReadMSH takes for triangles besides the 3-node one (Msh2Tri.F90:132-334): their
# extra nodes would have to follow the rotation; no fixture has them
OTHER_ACCEPTED = {9, 20, 21, 23, 24, 25}

ALL_TRIPLES = {(f, g, d) for f in (1, 2, 3) for g in (1, 2, 3) for d in (0, 1)}
ALL_PATTERNS = {(), (1,), (2,), (3,), (1, 2), (1, 3), (2, 3), (1, 2, 3)}

# the committed variants: name -> (source fixture, seed)
VARIANTS = {"untitled8_rn.msh": ("untitled8.msh", 1), "irregular_rn.msh": ("irregular.msh", 2),
            "test_sn2_rn.msh": ("test_sn2.msh", 3)}


def renumber(src, dst, seed, rotate=True, flip=True, permute=True):
    """Write `src` to `dst` with every triangle's node triple cyclically rotated (rotate), two of its
    nodes swapped for about half of the triangles (flip: the fixtures mix orientations already) and
    the triangles in another order (permute). Elements that are no triangles stay first, in their
    order; element ids run 1..n in the new order. Every other line is copied."""
    rng = np.random.default_rng(seed)
    with open(src) as f:
        lines = f.read().splitlines()
    start = next(i for i, s in enumerate(lines) if s.strip() == "$Elements")
    n = int(lines[start + 1])
    body = [s.split() for s in lines[start + 2:start + 2 + n]]
    assert lines[start + 2 + n].strip() == "$EndElements"
    others = [t for t in body if int(t[1]) != TRIANGLE]
    tris = [t for t in body if int(t[1]) == TRIANGLE]
    assert not any(int(t[1]) in OTHER_ACCEPTED for t in others), "higher-order triangles are not handled"
    # one draw of each kind per triangle whatever the switches, so that a switch changes only its own effect
    shifts = rng.integers(0, 3, len(tris))
    swaps = rng.integers(0, 2, len(tris))
    order = rng.permutation(len(tris))
    out = []
    for q in (order if permute else range(len(tris))):
        t = list(tris[q])
        at = 3 + int(t[2])
        nodes = t[at:at + 3]
        if rotate:
            s = int(shifts[q])
            nodes = nodes[s:] + nodes[:s]
        if flip and swaps[q]:
            nodes = [nodes[1], nodes[0], nodes[2]]
        out.append(t[:at] + nodes + t[at + 3:])
    new = [" ".join([str(i + 1)] + t[1:]) for i, t in enumerate(others + out)]
    with open(dst, "w") as f:
        f.write("\n".join(lines[:start + 2] + new + lines[start + 2 + n:]) + "\n")


def _tables(mesh):
    U = mesh.U
    return (np.asarray(mesh.neig).reshape(U, 3), np.asarray(mesh.fneig).reshape(U, 3),
            np.asarray(mesh.dir).reshape(U, 3))


def interface_triples(mesh):
    ne, fn, di = _tables(mesh)
    return {(int(f) + 1, int(fn[u, f]), int(di[u, f])) for u, f in zip(*np.nonzero(ne))}


def boundary_patterns(mesh):
    ne, _, _ = _tables(mesh)
    return {tuple(int(f) + 1 for f in np.flatnonzero(row == 0)) for row in ne}


def write_committed(meshes_dir):
    """(re)write the committed variants from their fixtures"""
    for name, (src, seed) in VARIANTS.items():
        renumber(os.path.join(meshes_dir, src), os.path.join(meshes_dir, name), seed)


if __name__ == "__main__":
    write_committed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "meshes"))
