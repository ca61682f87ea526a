"""Host side of the compact training path (uint8 image + uint8 class map -> x, seg, bound, dist, color on the GPU): the two facts
the kernels of csrc/targets.hip rest on, restated in numpy and pinned against labels.py; the loader's uint8 slots; the converter;
the CLI flags; the C ABI's argument checks (no launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import compact, labels
from resunet_a_mltsk_keras_amd.keras_api import compact_batch
from resunet_a_mltsk_keras_amd.loader import PrefetchLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_masks(rng, n):
    """0/1 masks: smooth blobs, salt-and-pepper noise, rectangles touching borders and corners, lines and single pixels."""
    out = []
    for k in range(n):
        H, W = int(rng.integers(3, 40)), int(rng.integers(3, 40))
        kind = k % 5
        if kind == 0:
            f = rng.random((H // 3 + 2, W // 3 + 2))
            m = np.kron(f, np.ones((3, 3)))[:H, :W] > rng.uniform(0.3, 0.7)
        elif kind == 1:
            m = rng.random((H, W)) < rng.uniform(0.05, 0.95)
        elif kind == 2:
            m = np.zeros((H, W), bool)
            for _ in range(3):
                i, j = int(rng.integers(0, H)), int(rng.integers(0, W))
                m[:i + 1 if rng.random() < 0.5 else None, j:] ^= True          # rectangles anchored at a border / corner
        elif kind == 3:
            m = np.zeros((H, W), bool)
            m[int(rng.integers(0, H)), :] = True
            m[:, int(rng.integers(0, W))] = True
            m[int(rng.integers(0, H)), int(rng.integers(0, W))] ^= True
        else:
            m = (np.add.outer(np.arange(H), np.arange(W)) % int(rng.integers(2, 4))) == 0
        out.append(m.astype(np.uint8))
    return out


def local_boundary(mask):
    """The rule tgt_bound computes: replicate-border Sobel, L1 magnitude, NMS against the zero-padded magnitude with the integer
    tan(22.5 deg) test, every survivor an edge (no hysteresis), 3x3 cross dilation that ignores the outside."""
    p = np.pad(mask.astype(np.int32), 1, mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    m = np.abs(dx) + np.abs(dy)
    mp = np.pad(m, 1)
    ax, ay = np.abs(dx), np.abs(dy) << 15
    tg22 = ax * 13573
    tg67 = tg22 + (ax << 16)
    d = np.where(ay < tg22, 0, np.where(ay > tg67, 1, np.where((dx ^ dy) < 0, 3, 2)))
    keep = [(m > mp[1:-1, :-2]) & (m >= mp[1:-1, 2:]), (m > mp[:-2, 1:-1]) & (m >= mp[2:, 1:-1]),
            (m > mp[:-2, :-2]) & (m > mp[2:, 2:]), (m > mp[:-2, 2:]) & (m > mp[2:, :-2])]
    e = np.pad((m > 0) & np.choose(d, keep), 1)
    b = e[1:-1, 1:-1] | e[1:-1, :-2] | e[1:-1, 2:] | e[:-2, 1:-1] | e[2:, 1:-1]
    return b.astype(np.float32), m


def test_boundary_is_a_local_stencil_on_masks():
    """Canny(0, 1) of a 0/1 mask needs no hysteresis: |dx| + |dy| is even, so every candidate is strong."""
    masks = random_masks(np.random.default_rng(0), 240)
    for k, m in enumerate(masks):
        got, mag = local_boundary(m)
        assert (mag % 2 == 0).all(), k
        ref = labels.dilate_cross3(labels.canny_u8(m, 0, 1)).astype(np.float32) / 255.0
        assert np.array_equal(got, ref), k
        assert np.array_equal(labels.canny_u8(m, 0, 1), labels.canny_u8(m, 0, 0)), k


def random_class_maps(rng, n, C):
    out = []
    for k in range(n):
        H, W = int(rng.integers(1, 28)), int(rng.integers(1, 28))
        if k % 4 == 0:
            cls = rng.integers(0, C + 2, (H, W))                                        # noise, with out-of-range values
        elif k % 4 == 1:
            f = rng.integers(0, C, (H // 4 + 2, W // 4 + 2))
            cls = np.kron(f, np.ones((4, 4), np.int64))[:H, :W]                       # blocks
        elif k % 4 == 2:
            cls = np.full((H, W), int(rng.integers(0, C)))                           # one class fills the patch
            cls[: int(rng.integers(0, H + 1)), : int(rng.integers(0, W + 1))] = 255
        else:
            cls = (np.add.outer(np.arange(H), 2 * np.arange(W)) // int(rng.integers(1, 6))) % (C + 1)
        out.append(cls.astype(np.uint8))
    return out


def distance_per_pixel(cls, C):
    """tgt_columns + tgt_rows + the normalisation of tgt_pixels: g = the distance along the column to the nearest other class
    value; d^2(i, j) = min_k (j - k)^2 + (cls(i, k) == cls(i, j) ? g(i, k)^2 : 0); d = float32(sqrt(float64 d^2));
    dist[p, c] = d(p) / max{d(q) : cls(q) = c} for c = cls(p) (0 for an absent class or one that fills the patch)."""
    H, W = cls.shape
    INF = 1 << 40
    g = np.full((H, W), INF, np.int64)
    rows = np.arange(H)
    for j in range(W):
        for i in range(H):
            other = rows[cls[:, j] != cls[i, j]]
            if other.size:
                g[i, j] = np.abs(other - i).min()
    g2 = np.where(g < INF, g * g, INF)
    d2 = np.empty((H, W), np.int64)
    ks = np.arange(W)
    for i in range(H):
        for j in range(W):
            d2[i, j] = ((ks - j) ** 2 + np.where(cls[i] == cls[i, j], g2[i], 0)).min()
    d = np.where(d2 < INF, np.sqrt(np.minimum(d2, INF - 1).astype(np.float64)).astype(np.float32), np.float32(0))
    out = np.zeros((H, W, C), np.float32)
    for c in range(C):
        sel = cls == c
        hi = d[sel].max() if sel.any() else np.float32(0)
        if hi > 0:
            out[..., c][sel] = d[sel] / hi
    return out


def test_one_distance_per_pixel_serves_every_class():
    rng = np.random.default_rng(1)
    for C in (1, 2, 6):
        for k, cls in enumerate(random_class_maps(rng, 24, C)):
            ref = labels.get_distance_label(compact.onehot(cls, C))
            got = distance_per_pixel(cls, C)
            assert got.dtype == ref.dtype and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (C, k)


def test_sqrt_of_integer_squares_is_scipys_distance():
    """d = float32(sqrt(float64(d^2))) is what distance_transform_edt gives (float64) cast to float32, for every squared distance
    a 512 x 512 patch can have; the float32 sqrt of the same integer agrees as well."""
    d2 = np.arange(0, 511 * 511 * 2 + 1, dtype=np.int64)
    a = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    assert np.array_equal(a, np.sqrt(d2.astype(np.float32)))


def make_reference_dataset(root, n=5, ps=12, C=4, norm_type=1, seed=0):
    """Patches in the reference's layout, the targets from labels.multitask_labels (what preprocess_save_patches_ISPRS.py writes)."""
    rng = np.random.default_rng(seed)
    for d in ["train", "labels/seg", "labels/bound", "labels/dist", "labels/color"]:
        os.makedirs(os.path.join(root, d), exist_ok=True)
    raw = {}
    for i in [3, 0, 4, 1, 2][:n]:
        name = f"patch_{i}.npy"
        rgb = rng.integers(0, 256, (ps, ps, 3)).astype(np.uint8)
        rgb[0, 0] = 255
        cls = np.kron(rng.integers(0, C, (ps // 3, ps // 3)), np.ones((3, 3), np.int64)).astype(np.uint8)
        img = rgb.astype(np.float32)
        img /= np.float32(compact.NORM_DIV[norm_type])
        t = labels.multitask_labels(compact.onehot(cls, C), rgb, norm_type)
        np.save(os.path.join(root, "train", name), img)
        for h, a in t.items():
            np.save(os.path.join(root, "labels", h, name), a)
        raw[name] = (rgb, cls, img, t)
    return raw


@pytest.mark.parametrize("norm_type", [1, 2])
def test_converter_round_trip_is_bit_exact(tmp_path, norm_type):
    src, dst = str(tmp_path / "ref"), str(tmp_path / "compact")
    raw = make_reference_dataset(src, norm_type=norm_type)
    assert compact.main(["--src", src, "--dst", dst, "--norm_type", str(norm_type)]) == 0
    assert sorted(os.listdir(os.path.join(dst, "images"))) == sorted(raw)
    assert not os.path.exists(os.path.join(dst, "labels", "bound"))
    for name, (rgb, cls, img, t) in raw.items():
        u8 = np.load(os.path.join(dst, "images", name))
        c8 = np.load(os.path.join(dst, "labels", "classes", name))
        assert u8.dtype == np.uint8 and c8.dtype == np.uint8
        assert np.array_equal(u8, rgb) and np.array_equal(c8, cls)
        host = compact.host_targets(u8[None], c8[None], 4, norm_type)
        assert np.array_equal(host["x"][0].view(np.uint32), img.view(np.uint32))
        for h in ("seg", "bound", "dist", "color"):
            assert np.array_equal(host[h][0].view(np.uint32), t[h].view(np.uint32)), h


def test_converter_refuses_what_uint8_cannot_represent(tmp_path):
    src = str(tmp_path / "ref")
    make_reference_dataset(src, n=2)
    p = os.path.join(src, "train", "patch_0.npy")
    img = np.load(p)
    img[1, 1, 0] = np.float32(0.5 / 255)
    np.save(p, img)
    with pytest.raises(ValueError, match="patch_0.npy"):
        compact.convert(src, str(tmp_path / "out"), 1)
    with pytest.raises(ValueError):                         # a norm_type 3 (standardised) image
        compact.image_to_u8(np.float32([[[-0.3, 0.1, 1.7]]]), 1)
    with pytest.raises(ValueError):                         # a norm_type 1 image read as norm_type 2
        compact.image_to_u8(np.float32([[[1 / 255, 0.0, 1.0]]]) / np.float32(1.0), 2)
    with pytest.raises(ValueError):
        compact.seg_to_classes(np.full((2, 2, 3), 0.5, np.float32))


def test_loader_keep_dtype_gives_uint8_slots_and_the_same_shard(tmp_path):
    src, dst = str(tmp_path / "ref"), str(tmp_path / "compact")
    make_reference_dataset(src, n=5)
    compact.convert(src, dst, 1)
    sys.path.insert(0, ROOT)
    import train_ISPRS as cli
    xs, ys = cli.list_compact_dataset(dst)
    order = [4, 2, 0, 1, 3]
    for rank in (0, 1):
        a = list(PrefetchLoader(xs, ys, 4, order=order, pin=False, rank=rank, world=2, keep_dtype=True))
        b = list(PrefetchLoader(xs, ys, 4, order=order, pin=False, rank=rank, world=2))
        assert len(a) == len(b) == 1
        (xa, ya), (xb, yb) = a[0], b[0]
        assert xa.dtype == torch.uint8 and ya["classes"].dtype == torch.uint8
        assert xb.dtype == torch.float32 and yb["classes"].dtype == torch.float32
        assert xa.shape == (2, 12, 12, 3) and ya["classes"].shape == (2, 12, 12)
        assert torch.equal(xa.float(), xb) and torch.equal(ya["classes"].float(), yb["classes"])
        want = [np.load(xs[i]) for i in order[rank * 2:rank * 2 + 2]]
        assert np.array_equal(xa.numpy(), np.stack(want))


def test_cli_compact_flags_and_listing(tmp_path):
    sys.path.insert(0, ROOT)
    import train_ISPRS as cli
    a = cli.build_parser().parse_args([])
    assert a.compact_dataset is False and a.norm_type == 1
    b = cli.build_parser().parse_args("--compact_dataset yes --norm_type 2 --multitasking yes".split())
    assert b.compact_dataset is True and b.norm_type == 2
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args("--norm_type 3".split())
    os.makedirs(tmp_path / "images")
    os.makedirs(tmp_path / "labels" / "classes")
    for i in [2, 0, 3, 1]:                                   # written in scrambled order
        np.save(tmp_path / "images" / f"p{i}.npy", np.full((4, 4, 3), i, np.uint8))
        np.save(tmp_path / "labels" / "classes" / f"p{i}.npy", np.full((4, 4), i, np.uint8))
    xs, ys = cli.list_compact_dataset(str(tmp_path))
    assert list(ys) == ["classes"]
    for x, y in zip(xs, ys["classes"]):
        assert os.path.basename(x) == os.path.basename(y) and np.load(x)[0, 0, 0] == np.load(y)[0, 0]
    x_tr, y_tr, x_va, y_va = cli.split_dataset(xs, ys)
    assert [os.path.basename(p) for p in x_tr] == [os.path.basename(p) for p in y_tr["classes"]]
    os.remove(tmp_path / "labels" / "classes" / "p3.npy")
    with pytest.raises(FileNotFoundError, match="p3.npy"):
        cli.list_compact_dataset(str(tmp_path))


def test_compact_batch_detection():
    x = np.zeros((2, 4, 4, 3), np.uint8)
    y = np.arange(32).reshape(2, 4, 4)                          # int64 in [0, 255]: converted
    cx, cy = compact_batch(x, y)
    assert cx is x and cy.dtype == np.uint8 and np.array_equal(cy, y)
    cx, cy = compact_batch(torch.from_numpy(x), torch.from_numpy(y).to(torch.int32))
    assert cy.dtype == torch.uint8
    assert compact_batch(x, y.astype(np.float32)) is None                        # float labels: the float path
    assert compact_batch(x, {"seg": y}) is None and compact_batch(x, None) is None
    assert compact_batch(x, np.zeros((2, 4, 4, 6), np.uint8)) is None             # one-hot: the float path
    with pytest.raises(ValueError, match=r"\[0, 255\]"):
        compact_batch(x, y - 1)
    with pytest.raises(ValueError, match="uint8"):
        compact_batch(x.astype(np.float32), y)
    with pytest.raises(ValueError):
        compact_batch(np.zeros((2, 4, 5, 3), np.uint8), y)


def test_targets_argument_validation_without_launch():
    """Every case breaks exactly one precondition of a valid call, so none of them reaches a launch."""
    lib = L.lib()
    fn = lib.raw("rua_multitask_targets")
    assert lib.raw("rua_targets_scratch_bytes")(8, 6) == 8 * 6 * 4
    A = 1 << 24                                               # fake, suitably aligned addresses: never dereferenced on the host
    ok = dict(img=A, cls=A, N=2, H=16, W=16, Cin=3, C=4, norm=1, x=A, seg=A, bound=A, dist=A, color=A, scratch=A, sb=2 * 4 * 4)
    bad = [
        (dict(img=None), b"required"), (dict(x=None), b"required"), (dict(cls=None), b"together"),
        (dict(bound=None), b"all null"), (dict(norm=3), b"norm_type"), (dict(norm=0), b"norm_type"),
        (dict(Cin=4), b"Cin = 3"), (dict(H=513), b"512"), (dict(W=0), b"512"), (dict(N=0), b"512"),
        (dict(C=0), b"num_classes"), (dict(C=65), b"num_classes"), (dict(x=A + 4), b"16-byte"),
        (dict(dist=A + 8), b"16-byte"), (dict(cls=A + 1), b"4-byte"), (dict(scratch=None), b"scratch"),
        (dict(sb=2 * 4 * 4 - 1), b"scratch"), (dict(scratch=A + 2), b"scratch"),
        (dict(N=40000, H=512, W=512), b"2^31"),
        (dict(bound=None, dist=None, color=None, Cin=17), b"Cin"),
    ]
    for change, msg in bad:
        a = dict(ok, **change)
        rc = fn(a["img"], a["cls"], a["N"], a["H"], a["W"], a["Cin"], a["C"], a["norm"], a["x"], a["seg"], a["bound"], a["dist"],
                a["color"], a["scratch"], a["sb"], None)
        assert rc == -1, change
        assert msg in lib.dll.rua_last_error(), (change, lib.dll.rua_last_error())
