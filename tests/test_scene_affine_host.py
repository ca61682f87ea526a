"""Host side of the affine scene windows (scenes.py: host_windows_affine, affine_rows, AffineSceneBatch, SceneLoader(jitter=);
csrc/scene.hip's argument checks; the CLI flags): the integer definition against host_windows for the eight symmetries, against
scipy's map_coordinates for free maps, the reflection rule on tiny scenes index by index, rua_scene_windows_affine's refusals
(no launch: safe without a GPU), and the loader's draws."""
import ctypes
import os
import sys

import numpy as np
import pytest
from scipy.ndimage import map_coordinates

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 65536


def scene(rng, H, W, C=3, classes=200):
    return rng.integers(0, 256, (H, W, C)).astype(np.uint8), rng.integers(0, classes, (H, W)).astype(np.uint8)


def border_rows(H, W, PH, PW, codes, rng, extra=6):
    """The four corners, a window on each border and `extra` random ones, under every code of `codes`."""
    r1, c1 = H - PH, W - PW
    spots = [(0, 0), (0, c1), (r1, 0), (r1, c1), (0, c1 // 2), (r1, c1 // 3), (r1 // 2, 0), (r1 // 3, c1)]
    spots += [(int(rng.integers(0, r1 + 1)), int(rng.integers(0, c1 + 1))) for _ in range(extra)]
    return np.array([[0, r, c, code] for r, c in spots for code in codes], np.int32)


# ---- 1. no jitter: the eight symmetries, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("PH,PW,codes", [(64, 64, list(range(8))), (37, 37, list(range(8))), (48, 80, [0, 2, 3, 4])])
@pytest.mark.parametrize("Cin", [1, 3, 7])
def test_affine_rows_without_jitter_reproduce_host_windows(PH, PW, codes, Cin):
    rng = np.random.default_rng(PH + PW + Cin)
    img, cls = scene(rng, 301, 333, Cin)                       # odd width
    rows4 = border_rows(301, 333, PH, PW, codes, rng)
    t7 = scenes.affine_rows(rows4, (PH, PW))
    assert t7.dtype == np.int32 and t7.shape == (len(rows4), 7)
    wi, wc = scenes.host_windows([img], [cls], rows4, (PH, PW))
    gi, gc = scenes.host_windows_affine([img], [cls], t7, (PH, PW))
    assert np.array_equal(gi, wi) and np.array_equal(gc, wc)
    oi, oc = scenes.host_windows_affine([img], None, t7, (PH, PW))
    assert oc is None and np.array_equal(oi, wi)
    # the matrices are the exact symmetry matrices and scenes.transform is what they reproduce
    for k, (s, r, c, code) in enumerate(rows4.tolist()):
        assert np.array_equal(t7[k, 3:].reshape(2, 2), Q * scenes.SYMMETRY[code])
        assert np.array_equal(gi[k], scenes.transform(img[r:r + PH, c:c + PW], code))
    if PH != PW:
        for code in scenes.TRANSPOSING:
            with pytest.raises(ValueError, match=f"row 1: code {code} transposes"):
                scenes.affine_rows(np.array([[0, 0, 0, 0], [0, 0, 0, code]], np.int32), (PH, PW))


# ---- 2. free maps against scipy ---------------------------------------------------------------------------------------------------
def random_maps(rng, n, H, W, P, outside):
    """n rows: any angle, zoom log-uniform in [0.25, 4], the patch centre anywhere from `outside` px outside the scene to inside."""
    rows4 = np.zeros((n, 4), np.int32)
    rows4[:, 3] = rng.integers(0, 8, n)
    zoom = np.exp(rng.uniform(np.log(0.25), np.log(4.0), n))
    zoom[:2] = [0.25, 4.0]
    cy, cx = rng.uniform(-outside, H + outside, n), rng.uniform(-outside, W + outside, n)
    cy[:4], cx[:4] = [-outside, H + outside, H / 2, 3.0], [W / 2, -outside, W + outside, 5.0]
    # affine_rows centres the patch on the centre of window (row 0, col 0): (P - 1) / 2; the shift moves it to (cy, cx)
    shift = np.stack([np.rint((cy - (P - 1) / 2) * Q), np.rint((cx - (P - 1) / 2) * Q)], 1).astype(np.int64)
    return scenes.affine_rows(rows4, P, rng.uniform(-180, 180, n), zoom, shift)


def test_against_scipy_map_coordinates():
    """Image: below 2.5 grey levels of order-1 'mirror' interpolation at the Q16 coordinates - each fraction is truncated to 8 bits,
    which moves less than 1/256 of weight per axis (less than 255 * 2 / 256, about 2, in all), plus 0.5 for the final rounding.
    Class map: order-0 sampling at floor(coordinate + 0.5), exactly."""
    rng = np.random.default_rng(20)
    H, W, P = 301, 333, 64
    img, cls = scene(rng, H, W, 3)
    t7 = random_maps(rng, 48, H, W, P, outside=40)
    assert len(t7) >= 40
    gi, gc = scenes.host_windows_affine([img], [cls], t7, P)
    i, j = np.arange(P, dtype=np.int64)[:, None], np.arange(P, dtype=np.int64)[None, :]
    worst, lo, hi = 0.0, 0.0, 0.0
    for k, (s, y0, x0, ayy, ayx, axy, axx) in enumerate(t7.tolist()):
        sy, sx = (y0 + i * ayy + j * ayx) / Q, (x0 + i * axy + j * axx) / Q
        lo, hi = min(lo, sy.min(), sx.min()), max(hi, (sy - H).max(), (sx - W).max())
        for ch in range(3):
            want = map_coordinates(img[..., ch].astype(np.float64), [sy, sx], order=1, mode="mirror")
            worst = max(worst, float(np.abs(gi[k, ..., ch] - want).max()))
        near = map_coordinates(cls, [np.floor(sy + 0.5), np.floor(sx + 0.5)], order=0, mode="mirror")
        assert np.array_equal(gc[k], near), k
    print(f"largest difference from map_coordinates(order=1, mode='mirror') over {len(t7)} maps: {worst:.3f} grey levels")
    assert lo < -40 and hi > 40                                # samples well outside the scene on both sides
    assert worst < 2.5


# ---- 3. the reflection rule on tiny scenes ----------------------------------------------------------------------------------------
def refl(t, n):
    m = 2 * (n - 1)
    u = t % m                                                  # Python's % is non-negative for m > 0
    return u if u < n else m - u


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5)])
def test_reflection_on_tiny_scenes_index_by_index(H, W):
    rng = np.random.default_rng(H * 10 + W)
    P = 64
    img, cls = scene(rng, H, W, 2)
    t7 = random_maps(rng, 6, H, W, P, outside=P)
    t7 = np.concatenate([t7, scenes.affine_rows(np.zeros((1, 4), np.int32), P, 0.0, 1.0, (-30 * Q, -17 * Q))])   # whole-pixel steps
    gi, gc = scenes.host_windows_affine([img], [cls], t7, P)
    for k, (s, y0, x0, ayy, ayx, axy, axx) in enumerate(t7.tolist()):
        for i in range(P):
            for j in range(P):
                sy, sx = y0 + i * ayy + j * ayx, x0 + i * axy + j * axx
                iy, ix, fy, fx = sy >> 16, sx >> 16, (sy & 0xFFFF) >> 8, (sx & 0xFFFF) >> 8
                for ch in range(2):
                    p = lambda r, c: int(img[refl(r, H), refl(c, W), ch])
                    v = ((256 - fy) * ((256 - fx) * p(iy, ix) + fx * p(iy, ix + 1)) + fy * ((256 - fx) * p(iy + 1, ix) + fx * p(iy + 1, ix + 1)) + 32768) >> 16
                    assert gi[k, i, j, ch] == v, (k, i, j, ch)
                assert gc[k, i, j] == cls[refl((sy + 32768) >> 16, H), refl((sx + 32768) >> 16, W)], (k, i, j)
    # np.pad's 'reflect' is the rule: the whole-pixel row reads the padded scene
    pad = np.pad(img, ((64, 64), (64, 64), (0, 0)), mode="reflect")
    assert np.array_equal(gi[-1], pad[64 - 30:64 - 30 + P, 64 - 17:64 - 17 + P])


# ---- 4. argument validation without a launch --------------------------------------------------------------------------------------
def test_affine_argument_validation_without_launch():
    """Every case breaks exactly one precondition of a valid call, so none of them reaches a launch; ScenePool.affine_batch refuses
    the same tables in the same words."""
    lib = L.lib()
    fn = lib.raw("rua_scene_windows_affine")
    A = 1 << 24                                               # fake, suitably aligned addresses: never dereferenced on the host
    shapes = [(40, 50), (64, 33)]
    n = len(shapes)
    ptrs = (ctypes.c_void_p * n)(A, A)
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)
    hs, ws = arr([s[0] for s in shapes]), arr([s[1] for s in shapes])
    good = np.array([[0, 8 * Q, 18 * Q, Q, 0, 0, Q], [1, -(1 << 30), 1 << 30, 4 * Q, -4 * Q, 4 * Q, -4 * Q], [0, 0, 0, 0, 0, 0, 0]], np.int32)

    def call(table, PH=32, PW=32, Cin=3, N=None, img_out=A, cls_out=A, scene_cls=ptrs, hs=hs, ws=ws):
        t = np.ascontiguousarray(table, dtype=np.int32)
        return fn(ptrs, scene_cls, hs, ws, n, t.ctypes.data, len(t) if N is None else N, PH, PW, Cin, img_out, cls_out, None)

    def pool_of(shapes, C=3):
        return scenes.ScenePool([np.zeros(s + (C,), np.uint8) for s in shapes], [np.zeros(s, np.uint8) for s in shapes], device="cpu")

    pool = pool_of(shapes)
    b = pool.affine_batch(good, 32)                            # the limits themselves are inside
    assert isinstance(b, scenes.AffineSceneBatch) and b.shape == (3, 32, 32, 3) and b.rows.dtype == np.int32

    general = [(dict(img_out=None), b"required"), (dict(cls_out=None), b"together"), (dict(scene_cls=None), b"together"),
               (dict(N=0), b"N 0"), (dict(Cin=17), b"Cin 17"), (dict(Cin=0), b"Cin 0"), (dict(PH=513), b"512"), (dict(PW=0), b"512"),
               (dict(img_out=A + 2), b"4-byte")]
    for change, msg in general:
        assert call(good, **change) == -1, change
        assert msg in lib.dll.rua_last_error() and b"rua_scene_windows_affine: " in lib.dll.rua_last_error(), (change, lib.dll.rua_last_error())
    for kw in (dict(PH=513), dict(PW=0)):                      # the patch limits: the same words from the pool
        assert call(good, **kw) == -1
        err = lib.dll.rua_last_error().decode()
        with pytest.raises(ValueError) as exc:
            pool.affine_batch(good, (kw.get("PH", 32), kw.get("PW", 32)))
        assert str(exc.value) == err
    with pytest.raises(ValueError, match="N 0"):
        pool.affine_batch(np.zeros((0, 7), np.int32), 32)
    with pytest.raises(ValueError, match=r"Cin 17 outside 1\.\.16"):
        scenes.check_affine_table(shapes, good, 32, 17)

    # scene sizes: 2 <= H, W <= 16384
    for bad_shapes in ([(40, 50), (1, 33)], [(40, 1), (64, 33)], [(40, 50), (16385, 33)], [(40, 16385), (64, 33)]):
        assert call(good, hs=arr([s[0] for s in bad_shapes]), ws=arr([s[1] for s in bad_shapes])) == -1
        err = lib.dll.rua_last_error().decode()
        s = 0 if bad_shapes[0] != shapes[0] else 1
        assert f"scene {s}: size {bad_shapes[s][0]} x {bad_shapes[s][1]} (2 <= H, W <= 16384)" in err, err
        with pytest.raises(ValueError) as exc:
            scenes.check_affine_table(bad_shapes, good, 32, 3)
        assert str(exc.value) == err
    scenes.check_affine_table([(2, 16384), (16384, 2)], good, 32, 3)                       # the limits themselves are inside

    O, M = 1 << 30, 4 * Q
    rows = [([2, 0, 0, Q, 0, 0, Q], "scene 2 outside 0..1"), ([-1, 0, 0, Q, 0, 0, Q], "scene -1 outside 0..1"),
            ([0, O + 1, 0, Q, 0, 0, Q], f"origin ({O + 1}, 0) outside -2^30..2^30"), ([0, -O - 1, 0, Q, 0, 0, Q], f"origin ({-O - 1}, 0) outside"),
            ([0, 0, O + 1, Q, 0, 0, Q], f"origin (0, {O + 1}) outside"), ([1, 0, -O - 1, Q, 0, 0, Q], f"origin (0, {-O - 1}) outside"),
            ([0, 0, 0, -2 ** 31, 0, 0, Q], f"coefficient {-2 ** 31} outside")]
    for q in range(4):
        for v in (M + 1, -M - 1):
            row = [0, 0, 0, Q, 0, 0, Q]
            row[3 + q] = v
            rows.append((row, f"coefficient {v} outside -262144..262144"))
    for at in (0, 2):                                          # the bad row first, and behind two good ones
        for row, msg in rows:
            table = np.concatenate([good[:at], np.array([row], np.int32)])
            assert call(table) == -1, row
            err = lib.dll.rua_last_error().decode()
            assert f"rua_scene_windows_affine: row {at}: " in err and msg in err, (row, err)
            with pytest.raises(ValueError) as exc:
                pool.affine_batch(table, 32)
            assert str(exc.value) == err, (str(exc.value), err)

    # the [N][4] entry points keep their words for a [N][7] table
    with pytest.raises(ValueError) as exc:
        pool.batch(good, 32)
    assert str(exc.value) == "a window table is an integer [N][4] array of (scene, row, col, code) rows, got int32 (3, 7)"
    with pytest.raises(ValueError, match=r"integer \[N\]\[7\] array"):
        pool.affine_batch(good[:, :4], 32)
    with pytest.raises(ValueError, match=r"integer \[N\]\[7\] array"):
        pool.affine_batch(good.astype(np.float32), 32)


# ---- 5. the loader ----------------------------------------------------------------------------------------------------------------
def test_scene_loader_with_a_jitter():
    rng = np.random.default_rng(50)
    sc = [scene(rng, 70, 90), scene(rng, 64, 40)]
    images, maps = [s[0] for s in sc], [s[1] for s in sc]
    pool = scenes.ScenePool(images, maps, patch=32, device="cpu")
    table = scenes.window_table(pool.shapes, 32, 8, True)
    order = np.random.default_rng(1).permutation(len(table))[:40]
    jit = scenes.Jitter(180.0, (0.75, 1.33), 4.0)

    def passes(n, **kw):
        ld = scenes.SceneLoader(pool, table, 8, order=order, jitter=jit, **kw)
        assert len(ld) == 5
        return [[b for b, none in ld if none is None] for _ in range(n)]

    a, b = passes(2, seed=3), passes(2, seed=3)
    assert all(len(p) == 5 and all(type(x) is scenes.AffineSceneBatch and x.rows.shape == (8, 7) for x in p) for p in a)
    for pa, pb in zip(a, b):                                   # the same seed: the same tables, pass by pass
        assert all(np.array_equal(x.rows, y.rows) for x, y in zip(pa, pb))
    assert all(not np.array_equal(x.rows, y.rows) for x, y in zip(a[0], a[1]))              # successive passes differ
    assert all(not np.array_equal(x.rows, y.rows) for x, y in zip(a[0], passes(1, seed=4)[0]))   # and so do seeds
    for p in a:
        for k, x in enumerate(p):
            scenes.check_affine_table(pool.shapes, x.rows, 32, 3)
            assert np.array_equal(x.rows[:, 0], table[order[k * 8:(k + 1) * 8], 0])         # the scenes of the loader's rows
    # pass 0, batch 1 is what the documented draws give
    angle, zoom, shift = jit.draw(np.random.default_rng([3, 0, 1]), 8)
    assert np.abs(angle).max() <= 180 and 0.75 <= zoom.min() and zoom.max() <= 1.33 and np.abs(shift).max() <= 4 * Q and shift.dtype == np.int64
    assert np.array_equal(a[0][1].rows, scenes.affine_rows(table[order[8:16]], 32, angle, zoom, shift))
    # a world of 2 sees the world-1 windows, row for row, in both passes
    r0, r1 = passes(2, seed=3, rank=0, world=2), passes(2, seed=3, rank=1, world=2)
    for e in range(2):
        for k in range(5):
            assert r0[e][k].rows.shape == (4, 7)
            assert np.array_equal(np.concatenate([r0[e][k].rows, r1[e][k].rows]), a[e][k].rows), (e, k)
            assert np.array_equal(a[e][k].shard(1, 2).rows, r1[e][k].rows) and type(a[e][k].shard(1, 2)) is scenes.AffineSceneBatch
    # slices keep the type and host() is host_windows_affine
    x = a[0][0]
    assert type(x[2:5]) is scenes.AffineSceneBatch and len(x[2:5]) == 3 and x.shape == (8, 32, 32, 3)
    hi, hc = x[2:5].host()
    wi, wc = scenes.host_windows_affine(images, maps, x.rows[2:5], 32)
    assert np.array_equal(hi, wi) and np.array_equal(hc, wc)
    with pytest.raises(TypeError):
        x[0]

    # without a jitter: plain SceneBatch objects with today's tables, every pass
    ld = scenes.SceneLoader(pool, table, 8, order=order, seed=3)
    for _ in range(2):
        got = list(ld)
        assert len(got) == 5
        for k, (sb, none) in enumerate(got):
            assert none is None and type(sb) is scenes.SceneBatch
            assert np.array_equal(sb.rows, table[order[k * 8:(k + 1) * 8]])
    with pytest.raises(ValueError, match="zoom range"):
        scenes.Jitter(10, (2.0, 1.0), 0)


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_random_aug_flags():
    sys.path.insert(0, ROOT)
    import train_ISPRS as cli
    a = cli.build_parser().parse_args([])
    assert a.random_aug is False and a.aug_rotate == 180 and list(a.aug_zoom) == [0.75, 1.33] and a.aug_shift is None
    assert a.scene_dataset is False and a.stride == 32 and a.data_aug is True              # the earlier defaults stand
    b = cli.build_parser().parse_args("--scene_dataset yes --random_aug yes --aug_rotate 30 --aug_zoom 0.5 2 --aug_shift 7.5".split())
    assert b.random_aug is True and b.aug_rotate == 30 and list(b.aug_zoom) == [0.5, 2.0] and b.aug_shift == 7.5
    with pytest.raises(SystemExit) as exc:
        cli.main("--resunet_a yes --random_aug yes".split())
    assert "--scene_dataset yes" in str(exc.value.code)
