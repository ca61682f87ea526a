"""Host side of training on partly labelled patches: the void mask's definition (labels.host_void_mask) against a brute-force double
loop, the margin that keeps the boundary target off the labelled side of a class / void interface, the converters that write
class 255 for "no class", the CLI flags and the refusals that need no device."""
import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import compact, labels, scenes
from resunet_a_mltsk_keras_amd.keras_api import void_margin

C = 4


def brute_void_mask(cls, num_classes, margin):
    N, H, W = cls.shape
    out = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        for i in range(H):
            for j in range(W):
                hit = False
                for a in range(i - margin, i + margin + 1):
                    for b in range(j - margin, j + margin + 1):
                        if 0 <= a < H and 0 <= b < W and cls[n, a, b] >= num_classes:
                            hit = True
                out[n, i, j] = 255 if hit else 0
    return out


def void_case(H, W, seed):
    """Three patches of classes 0..C-1 with void at the corners, sparse void bytes of the values C, 200 and 255, the whole last row of patch 0
    void and the first rows of patch 1 valid (a leak across patches would show there), patch 2 with a void blob in the middle."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, C, (3, H, W)).astype(np.uint8)
    cls[0, 0, 0], cls[0, 0, W - 1], cls[1, H - 1, 0], cls[1, H - 1, W - 1] = C, 200, 255, C
    cls[0, H - 1, :] = 255
    cls[2, H // 2, W // 3: W // 3 + 2] = [200, C]
    for v in (C, 200, 255):
        cls[2][rng.random((H, W)) < 0.01] = v
    return cls


@pytest.mark.parametrize("H,W", [(5, 7), (33, 64)])
@pytest.mark.parametrize("margin", [0, 1, 2, 16])
def test_host_void_mask_against_a_double_loop(H, W, margin):
    cls = void_case(H, W, H * 100 + W)
    got = labels.host_void_mask(cls, C, margin)
    assert got.dtype == np.uint8 and got.shape == cls.shape and set(np.unique(got)) <= {0, 255}
    assert np.array_equal(got, brute_void_mask(cls, C, margin))
    if margin == 0:
        assert np.array_equal(got, np.where(cls >= C, 255, 0))
    if margin < H - 1:                                         # patch 0's void last row does not reach into patch 1's first rows
        assert not got[1, 0].any() or (cls[1, :margin + 1] >= C).any()


def test_host_void_mask_refuses_bad_arguments():
    cls = np.zeros((1, 4, 4), np.uint8)
    for bad in (-1, 17, 1.0, True):
        with pytest.raises(ValueError, match="margin"):
            labels.host_void_mask(cls, C, bad)
    with pytest.raises(ValueError, match="uint8"):
        labels.host_void_mask(cls.astype(np.int32), C, 2)
    with pytest.raises(ValueError, match="uint8"):
        labels.host_void_mask(cls[0], C, 2)
    with pytest.raises(ValueError, match="num_classes"):
        labels.host_void_mask(cls, 256, 2)


def blob_void(seed, H=64, W=64):
    rng = np.random.default_rng(seed)
    f = rng.random((H // 4 + 2, W // 4 + 2))
    return np.kron(f, np.ones((4, 4)))[:H, :W] > rng.uniform(0.4, 0.7)


@pytest.mark.parametrize("seed", range(6))
def test_margin_two_keeps_the_boundary_target_off_the_valid_pixels(seed):
    """One class and a void blob: Canny + the 3x3 cross draw the class / void interface up to 2 pixels into the labelled side.  With the default
    margin no valid pixel carries a boundary target; over the seeds margin 1 leaves some (see the next test), so a too-small default would show."""
    void = blob_void(seed)
    assert void.any() and not void.all()
    cls = np.where(void, 255, 0).astype(np.uint8)
    bound = labels.get_boundary_label(compact.onehot(cls, C))
    assert labels.VOID_MARGIN == 2
    valid = labels.host_void_mask(cls[None], C, labels.VOID_MARGIN)[0] == 0
    assert valid.any()
    assert not bound[valid].any()


def test_margin_one_is_too_small():
    hits = 0
    for seed in range(6):
        cls = np.where(blob_void(seed), 255, 0).astype(np.uint8)
        bound = labels.get_boundary_label(compact.onehot(cls, C))
        hits += int(bound[labels.host_void_mask(cls[None], C, 1)[0] == 0].any())
    assert hits >= 1


def test_colours_to_classes_unknown_void():
    rng = np.random.default_rng(3)
    table = list(scenes.ISPRS_COLOURS.items())
    idx = rng.integers(0, len(table), (9, 11))
    ref = np.array([table[k][0] for k in idx.ravel()], np.uint8).reshape(9, 11, 3)
    want = np.array([table[k][1] for k in idx.ravel()], np.uint8).reshape(9, 11)
    assert np.array_equal(scenes.colours_to_classes(ref), want)
    assert np.array_equal(scenes.colours_to_classes(ref, unknown="void"), want)
    ref[4, 7] = ref[8, 10] = (255, 0, 0)                       # the benchmark's clutter: in neither colour table
    with pytest.raises(ValueError, match=r"unknown colour \(255, 0, 0\) at row 4, column 7"):
        scenes.colours_to_classes(ref)
    got = scenes.colours_to_classes(ref, unknown="void")
    want[4, 7] = want[8, 10] = 255
    assert np.array_equal(got, want)
    with pytest.raises(ValueError, match="'error' or 'void'"):
        scenes.colours_to_classes(ref, unknown="skip")
    img = rng.integers(0, 256, (3, 9, 11)).astype(np.uint8)
    assert np.array_equal(scenes.convert_reference_inputs(img, ref.transpose(2, 0, 1), unknown="void")[1], want)
    with pytest.raises(ValueError, match="unknown colour"):
        scenes.convert_reference_inputs(img, ref.transpose(2, 0, 1))


def test_scene_converter_cli_unknown_colour(tmp_path):
    rng = np.random.default_rng(4)
    ref = np.zeros((3, 70, 70), np.uint8)
    ref[:, :, :] = 255                                         # class 0 everywhere ...
    ref[:, 10:20, 30:40] = np.array([255, 0, 0], np.uint8)[:, None, None]      # ... and a clutter rectangle
    np.save(tmp_path / "img.npy", rng.integers(0, 256, (3, 70, 70)).astype(np.uint8))
    np.save(tmp_path / "ref.npy", ref)
    argv = ["--image", str(tmp_path / "img.npy"), "--reference", str(tmp_path / "ref.npy"), "--dst", str(tmp_path / "out")]
    with pytest.raises(ValueError, match="unknown colour"):
        scenes.main(argv)                                      # the default is today's behaviour
    assert scenes.main(argv + ["--unknown_colour", "void"]) == 0
    _, _, maps = scenes.load_scene_dir(str(tmp_path / "out"))
    assert (maps[0][10:20, 30:40] == 255).all() and (np.delete(maps[0], np.s_[10:20], 0) == 0).all()


def test_compact_converter_all_zero_rows():
    seg = np.eye(C, dtype=np.float32)[np.random.default_rng(5).integers(0, C, (6, 5))]
    want = seg.argmax(-1).astype(np.uint8)
    assert np.array_equal(compact.seg_to_classes(seg), want)
    assert np.array_equal(compact.seg_to_classes(seg, zero_rows_void=True), want)
    seg[2, 3] = 0
    with pytest.raises(ValueError, match="one-hot"):
        compact.seg_to_classes(seg)                            # the default still refuses
    want[2, 3] = 255
    assert np.array_equal(compact.seg_to_classes(seg, zero_rows_void=True), want)
    seg[0, 0] = 1                                              # two ones in a row: refused either way
    with pytest.raises(ValueError, match="one-hot"):
        compact.seg_to_classes(seg, zero_rows_void=True)
    # the class map of such a label gives back the label: an all-zero row for 255
    assert np.array_equal(compact.onehot(want, C)[2, 3], np.zeros(C, np.float32))


def test_train_cli_void_flags():
    import train_ISPRS as cli
    a = cli.build_parser().parse_args([])
    assert a.ignore_void is False and a.void_margin == 2 and cli.check_void_flags(a) is None
    a = cli.build_parser().parse_args("--void_margin 5".split())
    assert cli.check_void_flags(a) is None                     # the margin alone switches nothing on
    for layout in ("--compact_dataset", "--scene_dataset"):
        a = cli.build_parser().parse_args(["--ignore_void", "yes", layout, "yes"])
        assert cli.check_void_flags(a) == 2
        a = cli.build_parser().parse_args(["--ignore_void", "yes", layout, "yes", "--void_margin", "0"])
        assert cli.check_void_flags(a) == 0
    with pytest.raises(SystemExit) as exc:
        cli.check_void_flags(cli.build_parser().parse_args("--ignore_void yes".split()))
    assert "--compact_dataset yes or --scene_dataset yes" in str(exc.value)
    with pytest.raises(SystemExit) as exc:
        cli.main("--resunet_a yes --ignore_void yes".split())  # refused before anything is loaded
    assert "float layout" in str(exc.value)
    for bad in ("17", "-1"):
        with pytest.raises(SystemExit) as exc:
            cli.check_void_flags(cli.build_parser().parse_args(["--ignore_void", "yes", "--scene_dataset", "yes", "--void_margin", bad]))
        assert "0..16" in str(exc.value)
    with pytest.raises(SystemExit) as exc:
        cli.check_void_flags(cli.build_parser().parse_args("--ignore_void yes --compact_dataset yes -cp x.h5".split()))
    assert "checkpoint" in str(exc.value)


def test_compile_option_values():
    assert void_margin(None) is None and void_margin(False) is None
    assert void_margin(True) == labels.VOID_MARGIN == 2
    assert void_margin(0) == 0 and void_margin(16) == 16 and void_margin(np.int64(3)) == 3
    for bad in (17, -1, 2.0, "yes"):
        with pytest.raises(ValueError, match="ignore_void"):
            void_margin(bad)


def test_loss_spec_default_is_off():
    from resunet_a_mltsk_keras_amd.engine import LossSpec
    assert LossSpec().ignore_void is None
