"""CPU tests of the outlines' host side (scenes.host_outlines, host_outlines_jumping, outline_polygons, simplify_ring, write_geojson):
hand-written answers, and on random maps the properties that make rings an outline - rasterised back even-odd they give exactly the
id's pixels, their areas sum to the pixel counts, consecutive vertices alternate between sharing a row and sharing a column, leaders
ascend."""
import json

import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import scenes


def nested():
    """the 5 x 5 square of id 0 with a 3 x 3 hole and an island of the same id in it"""
    m = np.zeros((5, 5), np.int32)
    m[1:4, 1:4] = -1
    m[2, 2] = 0
    return m


def diagonal():
    return np.array([[0, -1], [-1, 0]], np.int32)


def serpentine(H, W, ident=0):
    """a one-pixel path: every other row full, joined at alternating ends"""
    m = np.full((H, W), -1, np.int32)
    m[::2] = ident
    for k, i in enumerate(range(1, H - 1 if H % 2 else H, 2)):
        m[i, -1 if k % 2 == 0 else 0] = ident
    return m


def rasterise(ring_list, H, W):
    """even-odd: a pixel is inside if an odd number of vertical ring edges lie east of its centre"""
    hit = np.zeros((H, W), np.int64)
    for ring in ring_list:
        for (y0, x0), (y1, x1) in zip(ring, np.roll(ring, -1, 0)):
            if x0 == x1:
                hit[min(y0, y1):max(y0, y1), :x0] += 1
    return hit % 2 == 1


def rings_of(rings, verts):
    return [verts[r[2]:r[2] + r[3]] for r in rings]


def check_properties(m, conn):
    H, W = m.shape
    rings, verts = scenes.host_outlines(m, conn)
    assert rings.dtype == np.int32 and verts.dtype == np.int32 and rings.shape[1:] == (6,) and verts.shape[1:] == (2,)
    assert (np.diff(rings[:, 1]) > 0).all(), "leaders ascend"
    assert np.array_equal(rings[:, 2], np.cumsum(rings[:, 3]) - rings[:, 3]) and rings[:, 3].sum() == len(verts)
    assert (rings[:, 3] >= 4).all() and (rings[:, 3] % 2 == 0).all() and (rings[:, 5] >= rings[:, 3]).all()
    each = rings_of(rings, verts)
    for ring in each:
        same_row, same_col = ring[:, 0] == np.roll(ring[:, 0], -1), ring[:, 1] == np.roll(ring[:, 1], -1)
        assert (same_row != same_col).all() and (same_row != np.roll(same_row, 1)).all(), "rows and columns alternate: no collinear point"
    for k in np.unique(m[m >= 0]):
        mine = rings[:, 0] == k
        assert np.array_equal(rasterise([r for r, ok in zip(each, mine) if ok], H, W), m == k), (conn, int(k))
        assert rings[mine, 4].sum() == (m == k).sum()
    assert set(rings[:, 0].tolist()) == set(m[m >= 0].tolist())
    again = scenes.host_outlines_jumping(m, conn)
    assert np.array_equal(again[0], rings) and np.array_equal(again[1], verts) and again[0].dtype == np.int32 and again[1].dtype == np.int32
    return rings, verts


def test_a_single_pixel():
    rings, verts = scenes.host_outlines(np.zeros((1, 1), np.int32))
    assert rings.tolist() == [[0, 0, 0, 4, 1, 4]] and verts.tolist() == [[0, 1], [1, 1], [1, 0], [0, 0]]
    rings, verts = scenes.host_outlines(np.full((1, 1), -3, np.int32))
    assert rings.shape == (0, 6) and verts.shape == (0, 2) and rings.dtype == np.int32


def test_the_nested_square():
    for conn in (4, 8):
        rings, verts = check_properties(nested(), conn)
        assert rings.tolist() == [[0, 0, 0, 4, 25, 20], [0, 6, 4, 4, -9, 12], [0, 48, 8, 4, 1, 4]]
        assert verts[:4].tolist() == [[0, 5], [5, 5], [5, 0], [0, 0]]
        assert verts[4:8].tolist() == [[1, 1], [4, 1], [4, 4], [1, 4]]                   # the hole runs the other way
        assert verts[8:].tolist() == [[2, 3], [3, 3], [3, 2], [2, 2]]


def test_the_diagonal_under_both_connectivities():
    rings, verts = check_properties(diagonal(), 4)
    assert rings.tolist() == [[0, 0, 0, 4, 1, 4], [0, 12, 4, 4, 1, 4]]
    rings, verts = check_properties(diagonal(), 8)
    assert rings.tolist() == [[0, 0, 0, 8, 2, 8]]
    assert verts.tolist() == [[0, 1], [1, 1], [1, 2], [2, 2], [2, 1], [1, 1], [1, 0], [0, 0]]
    other = np.array([[-1, 5], [5, -1]], np.int32)                                          # the other diagonal
    assert scenes.host_outlines(other, 8)[0].tolist() == [[5, 4, 0, 8, 2, 8]] and len(check_properties(other, 4)[0]) == 2


def test_properties_on_random_maps():
    rng = np.random.default_rng(3)
    for _ in range(120):
        H, W = (int(v) for v in rng.integers(1, 13, 2))
        m = rng.integers(-1, 4, (H, W)).astype(np.int32)
        for conn in (4, 8):
            check_properties(m, conn)
    blocks = np.kron(rng.integers(-1, 3, (4, 5)), np.ones((3, 3), np.int64)).astype(np.int32)
    for conn in (4, 8):
        check_properties(blocks, conn)


def test_a_serpentine_is_one_long_ring_and_ids_may_be_large():
    m = serpentine(9, 11, 2**31 - 1)
    rings, verts = check_properties(m, 4)
    assert len(rings) == 1 and rings[0, 0] == 2**31 - 1 and rings[0, 4] == (m >= 0).sum() and rings[0, 5] == 2 * (m >= 0).sum() + 2


def test_refusals():
    for bad, text in ((np.zeros((2, 2), np.int64), "int32 H x W"), (np.zeros((0, 2), np.int32), "int32 H x W"), (np.zeros(4, np.int32), "int32 H x W")):
        with pytest.raises(ValueError, match=text):
            scenes.host_outlines(bad)
    with pytest.raises(ValueError, match="connectivity 5 is neither 4 nor 8"):
        scenes.host_outlines(np.zeros((2, 2), np.int32), 5)
    with pytest.raises(ValueError, match=r"size 32768 x 16385 \(1 <= H, W and H \* W <= 2\^29"):
        scenes.check_outlines((32768, 16385))
    assert scenes.check_outlines((32768, 16384), 8) == (32768, 16384, 8)


def test_polygons_assign_holes_to_the_smallest_ring_round_them():
    m = np.full((11, 12), -1, np.int32)
    m[0:9, 0:9] = 0                                                                         # a square of id 0 ...
    m[1:8, 1:8] = -1                                                                        # ... with a hole ...
    m[2:7, 2:7] = 0                                                                         # ... an island of the same id in it ...
    m[3:6, 3:6] = 1                                                                         # ... whose own hole is filled by id 1 ...
    m[4, 4] = -1                                                                            # ... which has a hole too
    m[10, 0:3] = 1                                                                          # a second piece of id 1
    rings, verts = scenes.host_outlines(m)
    table = np.zeros((2, 8), np.int32)
    table[:, 1] = [3, 2]
    polys = scenes.outline_polygons(rings, verts, table)
    got = [(p["id"], p["class"], p["area"], len(p["holes"])) for p in polys]
    assert got == [(0, 3, 32, 1), (0, 3, 16, 1), (1, 2, 8, 1), (1, 2, 3, 0)]
    assert polys[0]["holes"][0].tolist() == [[1, 1], [8, 1], [8, 8], [1, 8]] and polys[1]["holes"][0].tolist() == [[3, 3], [6, 3], [6, 6], [3, 6]]
    assert polys[2]["holes"][0].tolist() == [[4, 4], [5, 4], [5, 5], [4, 5]] and polys[2]["exterior"].dtype == np.int32
    assert [p["area"] for p in scenes.outline_polygons(rings, verts, min_area=8)] == [32, 16, 8]
    assert scenes.outline_polygons(rings, verts)[0]["class"] is None
    nest = scenes.outline_polygons(*scenes.host_outlines(nested()))
    assert [(p["area"], len(p["holes"])) for p in nest] == [(16, 1), (1, 0)]
    assert scenes.outline_polygons(np.zeros((0, 6), np.int32), np.zeros((0, 2), np.int32)) == []
    with pytest.raises(ValueError, match="do not tile"):
        scenes.outline_polygons(rings, verts[:-1])


def test_simplify_ring():
    m = np.zeros((6, 10), np.int32)
    m[3, 9] = -1                                                                            # a one-pixel notch in the right side
    rings, verts = scenes.host_outlines(m)
    assert len(rings) == 1 and len(verts) == 8
    assert scenes.simplify_ring(verts, 0) is verts or np.array_equal(scenes.simplify_ring(verts, 0), verts)
    assert scenes.simplify_ring(verts, 1.5).tolist() == [[0, 10], [6, 10], [6, 0], [0, 0]]
    assert np.array_equal(scenes.simplify_ring(verts, 0.2), verts)                           # the notch is one pixel deep
    assert np.array_equal(scenes.simplify_ring(verts, 1.0), verts[[0, 5, 6, 7]])             # the test is <=
    square = scenes.host_outlines(np.zeros((1, 1), np.int32))[1]
    for tol in (0.5, 3, 1000):
        assert np.array_equal(scenes.simplify_ring(square, tol), square)
        assert len(scenes.simplify_ring(verts, tol)) >= 4
    ell = scenes.host_outlines(np.array([[0, -1], [0, 0]], np.int32))[1]                    # six vertices: three would be left
    assert len(ell) == 6 and np.array_equal(scenes.simplify_ring(ell, 5), ell)
    rng = np.random.default_rng(11)
    blob = np.kron(rng.integers(0, 2, (6, 6)), np.ones((4, 4), np.int64)).astype(np.int32) - 1
    for ring in rings_of(*scenes.host_outlines(blob, 8)):
        for tol in (0.5, 2, 4):
            out = scenes.simplify_ring(ring, tol)
            assert 4 <= len(out) <= len(ring) and out[0].tolist() == ring[0].tolist()
            assert all(any((v == w).all() for w in ring) for v in out)                    # a subset of the input, in order
    with pytest.raises(ValueError, match="at least 4 vertices"):
        scenes.simplify_ring(verts[:3], 1)
    with pytest.raises(ValueError, match="negative"):
        scenes.simplify_ring(verts, -1)


def area2(ring):
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(ring[:-1], ring[1:]))


def test_geojson_round_trip_and_orientation(tmp_path):
    polys = scenes.outline_polygons(*scenes.host_outlines(nested()))
    path = str(tmp_path / "p.geojson")
    assert scenes.write_geojson(path, polys, properties={"scene": "a"}) == 2
    with open(path) as f:
        doc = json.load(f)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == 2
    first = doc["features"][0]
    assert first["type"] == "Feature" and first["properties"] == {"id": 0, "class": None, "area": 16, "scene": "a"}
    outer, hole = first["geometry"]["coordinates"]
    assert first["geometry"]["type"] == "Polygon" and outer[0] == outer[-1] and hole[0] == hole[-1] and len(outer) == 5 and len(hole) == 5
    assert area2(outer) == 2 * 25 and area2(hole) == -2 * 9                              # counter-clockwise outside, clockwise inside
    assert sorted(map(tuple, outer[:-1])) == [(0, -5), (0, 0), (5, -5), (5, 0)]         # (y, x) -> (x, -y)
    # a transform that does not flip: the orientation follows the signed area after it
    scenes.write_geojson(path, polys, transform=(100.0, 0.5, 0.0, 200.0, 0.0, 0.5), properties=lambda p: {"holes": len(p["holes"])})
    with open(path) as f:
        doc = json.load(f)
    outer, hole = doc["features"][0]["geometry"]["coordinates"]
    assert area2(outer) == 2 * 25 * 0.25 and area2(hole) == -2 * 9 * 0.25 and [100.0, 200.0] in outer and [102.5, 202.5] in outer
    assert doc["features"][0]["properties"]["holes"] == 1 and doc["features"][1]["properties"]["holes"] == 0
    with pytest.raises(ValueError, match="six numbers"):
        scenes.write_geojson(path, polys, transform=(0, 1, 0))
