"""The light-centred shadow grid (csrc/shadow_grid.cpp), built on the host through hprt_debug_shadow_grid_build — no GPU.

The grid must hand k_shadow_grid a superset of the triangles a shadow ray can be reported to hit.  Checked from the geometry: for
every triangle and 64 points on it — and those points moved by the build's ε along every axis — the cell that the device computes
for the direction light -> point lists the triangle with a key no larger than the point's squared distance from the light and a
sub-cell rectangle that holds the point's sixteenth of the cell, or the near list holds the triangle.  Lists are sorted by key; the near list is what each scene predicts and never more than 1 % of a
scene that was not built to populate it."""
import numpy as np
import pytest

import shadow_grid_cases as sgc

SCENES = sgc.scenes()
RES = (8, 64, 512)


@pytest.fixture(scope="module")
def grids(hprt):
    out = {}
    for name, (text, _) in SCENES.items():
        p9 = sgc.text_triangles(text)
        for R in RES:
            out[name, R] = (p9, sgc.text_light(text), hprt.shadow_grid_build(p9, sgc.text_light(text), R))
    return out


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_point_of_a_triangle_finds_it_in_its_cell(grids, name, R):
    p9, L, g = grids[name, R]
    assert g["R"] == R
    n = p9.shape[0]
    tri = p9.reshape(n, 3, 3).astype(np.float64)
    pts = np.einsum("kv,nvc->nkc", sgc.triangle_points(), tri)                      # [n, 64, 3]
    eps = g["eps"]
    moves = np.concatenate([np.zeros((1, 3)), eps * np.eye(3), -eps * np.eye(3)])   # the point itself, +- eps along each axis
    in_near = np.zeros(n, bool)
    in_near[g["prim"][:g["near"]]] = True
    cs = g["cell_start"].astype(np.int64)
    # every (cell, triangle) pair of the lists -> its key, looked up through one sorted array
    cell_of_entry = np.searchsorted(cs, np.arange(g["near"], g["prim"].size), side="right") - 1
    pair = cell_of_entry * n + g["prim"][g["near"]:]
    order = np.argsort(pair)
    pair, key, rect = pair[order], g["key"][g["near"]:][order].astype(np.float64), g["rect"][g["near"]:][order]
    assert np.all(np.diff(pair) > 0)                                                # a triangle appears once in a cell
    who = np.repeat(np.arange(n), pts.shape[1])
    for mv in moves:
        q = (pts + mv).reshape(-1, 3)
        rel = q - L.astype(np.float64)
        # the direction of a ray that ends at the light and passes through q is (a positive multiple of) light - q
        cell, su, sv = sgc.cell_of((-rel).astype(np.float32), R)
        want = cell * n + who
        at = np.minimum(np.searchsorted(pair, want), pair.size - 1)
        found = pair[at] == want
        r = rect[at]
        reached = (r[:, 0] <= su) & (su <= r[:, 1]) & (r[:, 2] <= sv) & (sv <= r[:, 3])      # the entry reaches the point's sixteenth of the cell
        ok = in_near[who] | (found & reached & (key[at] <= (rel * rel).sum(1)))
        assert ok.all(), (name, R, int((~ok).sum()), who[~ok][:5], q[~ok][:2])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_lists_are_sorted_and_the_near_list_is_as_predicted(grids, name):
    for R in RES:
        p9, L, g = grids[name, R]
        cs = g["cell_start"].astype(np.int64)
        assert cs[0] == g["near"] and cs[-1] == g["prim"].size and np.all(np.diff(cs) >= 0)
        assert int(np.diff(cs).max()) == g["longest"]
        k = g["key"]
        assert np.all(k >= 0) and np.all(k[:g["near"]] == 0) and np.all(g["rect"][:g["near"]] == [0, 15, 0, 15])
        assert np.all(g["rect"][:, 0] <= g["rect"][:, 1]) and np.all(g["rect"][:, 2] <= g["rect"][:, 3])
        rising = np.diff(k[g["near"]:]) >= 0
        starts = cs[1:-1] - g["near"] - 1                                           # the step from one cell's last entry to the next cell's first
        rising[starts[(starts >= 0) & (starts < rising.size)]] = True
        assert rising.all()
        assert g["single"].all()                                                    # the hook makes every triangle a leaf of its own
        near = set(int(i) for i in g["prim"][:g["near"]])
        if SCENES[name][1] == "empty":
            assert near == set()
        else:
            # the scene built to populate it: the triangle 1e-4 from the light, the one with two equal vertices, the collinear one
            assert near == {0, 1, 2}
        if name != "near":
            assert len(near) <= 0.01 * p9.shape[0]

