// The tables of marching tetrahedra on the Kuhn subdivision (mesh.extract_mesh_reference is the definition).  csrc/isosurface.hip
// compiles them; nerf-pytorch_amd/mesh.py parses this file, so the kernels and the reference read the same numbers.  Plain int arrays
// with brace initialisers and nothing else: keep it that way.
#pragma once

// One tetrahedron per permutation (a, b, c) of the axes (0 = x, 1 = y, 2 = z): its corners in the unit cube are v0 = 0, v1 = e_a,
// v2 = e_a + e_b, v3 = (1, 1, 1).  det[v1 - v0, v2 - v0, v3 - v0] is the permutation's sign: rows 0, 3 and 4 are even.
constexpr int ISO_PERMS[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// The seven directions of a lattice edge, from its lower to its upper endpoint; edge id = 7 * node(lower endpoint) + class.
constexpr int ISO_CLASS_DIRS[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};

// The six edges of a tetrahedron as (lower corner, upper corner).
constexpr int ISO_TET_EDGES[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};

// Per inside mask (bit i: corner v_i is inside) of an EVEN tetrahedron: the number of triangles, then two triangles as rows of
// ISO_TET_EDGES, wound so that (p1 - p0) x (p2 - p0) points from the inside corners to the outside ones.  A quad (two inside) is
// (q0, q1, q2), (q0, q2, q3).  An odd tetrahedron is the mirror image: it swaps the last two corners of every triangle.
constexpr int ISO_TET_TRIS[16][7] = {
    {0, 0, 0, 0, 0, 0, 0},
    {1, 0, 1, 2, 0, 0, 0},
    {1, 0, 4, 3, 0, 0, 0},
    {2, 1, 2, 4, 1, 4, 3},
    {1, 1, 3, 5, 0, 0, 0},
    {2, 0, 3, 5, 0, 5, 2},
    {2, 0, 4, 5, 0, 5, 1},
    {1, 2, 4, 5, 0, 0, 0},
    {1, 2, 5, 4, 0, 0, 0},
    {2, 0, 1, 5, 0, 5, 4},
    {2, 0, 2, 5, 0, 5, 3},
    {1, 1, 5, 3, 0, 0, 0},
    {2, 1, 3, 4, 1, 4, 2},
    {1, 0, 3, 4, 0, 0, 0},
    {1, 0, 2, 1, 0, 0, 0},
    {0, 0, 0, 0, 0, 0, 0}};
