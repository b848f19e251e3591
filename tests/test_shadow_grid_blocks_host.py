"""The device image of the light-centred shadow grid (csrc/shadow_grid.h, ShadowGridImage), packed on the host through
hprt_debug_shadow_grid_image — no GPU.

The image must say exactly what the logical grid says (hprt_debug_shadow_grid_build, tests/test_shadow_grid_host.py): following a
cell as k_shadow_grid does — the block's head, its two slots, then the run of 48-byte records the head points to — gives the cell's
list, entry for entry: the same primitive words, key words (key and rectangle) and order, and vertex floats that are the triangle
records' bit for bit; the near list, records 0 .. near - 1, likewise.  The words a ray decides by before it fetches the next entry
(the block's copy of entry 2's key word, a record's copy of its successor's) are copies of those entries' own.  No read the kernel
can form — seven 16-byte words of a block, three of a record — leaves the image.

R = 1 makes every list far longer than a block, R = 8 and 64 give cells with 0, 1, 2 (the block alone, exactly full) and 3 entries
(one record); asserted below."""
import numpy as np
import pytest

import shadow_grid_cases as sgc

SCENES = sgc.scenes()
RES = (1, 8, 64)
SG_RECT_ALL = 0xf0f0


@pytest.fixture(scope="module")
def images(hprt):
    out = {}
    for name, (text, _) in SCENES.items():
        p9 = sgc.text_triangles(text)
        L = sgc.text_light(text)
        for R in RES:
            out[name, R] = (p9, hprt.shadow_grid_build(p9, L, R), hprt.shadow_grid_image(p9, L, R))
    return out


def _logical_words(g, hprt):
    prim = (g["prim"].astype(np.uint32) | np.where(g["single"], np.uint32(hprt.SG_SINGLE), np.uint32(0))).astype(np.uint32)
    r = g["rect"].astype(np.uint32)
    key = (g["key"].view(np.uint32) | r[:, 0] | (r[:, 1] << 4) | (r[:, 2] << 8) | (r[:, 3] << 12)).astype(np.uint32)
    return prim, key


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_decoding_every_cell_gives_the_logical_list(hprt, images, name, R):
    p9, g, im = images[name, R]
    assert g["R"] == R
    prim, key = _logical_words(g, hprt)
    cs = g["cell_start"].astype(np.int64)
    # the same lists: counts (so the same cell boundaries), then every entry's two words, in order
    assert np.array_equal(im["count"], np.diff(cs))
    assert np.array_equal(im["cell_start"], cs)
    assert np.array_equal(im["prim_word"], prim)
    assert np.array_equal(im["key_word"], key)
    # vertex floats: the triangle records', as uint32
    assert np.array_equal(im["verts"], p9.view(np.uint32)[g["prim"]])
    # the near list is the first `near` records, keys 0 and the whole cell
    near = g["near"]
    assert np.array_equal(im["records"][:near, 3], prim[:near]) and np.all(im["key_word"][:near] == SG_RECT_ALL)


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_runs_are_contiguous_and_the_look_ahead_words_are_copies(hprt, images, name, R):
    p9, g, im = images[name, R]
    _, key = _logical_words(g, hprt)
    cs = g["cell_start"].astype(np.int64)
    count, near = im["count"], g["near"]
    over = np.maximum(count - hprt.SG_BLOCK_SLOTS, 0)
    # one run per cell, in cell order, right behind the near list and each other
    assert np.array_equal(im["overflow"][over > 0], (near + np.cumsum(over) - over)[over > 0])
    n_records = near + int(over.sum())
    assert im["records"].shape[0] == n_records + 1 and not im["records"][n_records:].any()      # (the padding: one record of zeros)
    # the block's copy of entry 2's key word; 0 where the list has no third entry
    has3 = count > 2
    assert np.array_equal(im["key2"][has3], key[cs[:-1][has3] + 2]) and not im["key2"][~has3].any()
    # a record's fourth lane of its third word: the key word of the next entry of the same run, 0 behind the last
    for a, b in [(0, near)] + [(int(cs[c]) + 2, int(cs[c + 1])) for c in np.nonzero(has3)[0][:2000]]:
        if b > a:
            assert np.array_equal(im["next_key"][a:b - 1], key[a + 1:b]) and im["next_key"][b - 1] == 0
    # words of entries a list does not have, the spare lanes and the eighth word are 0
    b = im["blocks"]
    assert not b[count < 1][:, 2:16].any() and not b[count < 2][:, [7, 11]].any() and not b[count < 2][:, 16:].any()
    assert not b[:, [19, 23, 27, 28, 29, 30, 31]].any()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_cells_with_0_1_2_3_and_longest_entries_occur(images, name):
    seen = set()
    for R in RES:
        _, g, im = images[name, R]
        assert int(im["count"].max()) == g["longest"] > 3
        seen |= set(np.unique(im["count"]).tolist())
    # (the atrium is closed around its light: no direction without a wall, and where walls meet never fewer than two candidates)
    assert ({2, 3} if name == "atrium" else {0, 1, 2, 3}) <= seen, sorted(seen)[:8]
    # R = 1: six cells share the scene's triangles (300 in the smallest): the longest list is far past a block's two
    assert int(images[name, 1][2]["count"].max()) >= 50


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_no_read_of_the_kernel_leaves_the_image(hprt, images, name, R):
    """k_shadow_grid reads words 0 - 6 of the block at cell * 128 and the three words of the record at 48 * (overflow + i - 2) for
    2 <= i < count (the near list: 48 * i, i < near); blocks and records lie one behind the other in one buffer."""
    _, g, im = images[name, R]
    block_bytes, record_bytes = 4 * im["blocks"].size, 4 * im["records"].size
    assert im["words"] == (im["blocks"].size, im["records"].size, im["blocks"].size + im["records"].size)
    assert block_bytes == 6 * R * R * 128 and block_bytes % 128 == 0
    last_cell = 6 * R * R - 1
    assert last_cell * 128 + 7 * 16 <= block_bytes
    over = np.maximum(im["count"] - hprt.SG_BLOCK_SLOTS, 0)
    last = np.where(over > 0, im["overflow"] + over - 1, -1)
    assert (int(last.max()) + 1) * 48 <= record_bytes - 48 and g["near"] * 48 <= record_bytes - 48      # (inside, before the padding)
    assert block_bytes + record_bytes < 2 ** 32
