"""Host tests of the copy-paste augmentation: scenes.host_object_bank on hand-drawn maps, scenes.host_paste against hand-written
answers, check_paste_table word by word, paste_rows and CopyPaste.draw, SceneBatch / AffineSceneBatch carrying a paste table,
SceneLoader(paste=).  Nothing here touches a GPU: the pools are "cpu" pools."""
import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import scenes

ALL = -1                                                     # both onto words of "every class"


def row(window, scene, id_, code, top, left, i0, j0, h, w, lo=ALL, hi=ALL, flags=0):
    return [window, scene, id_, code, top, left, i0, j0, h, w, lo, hi, flags, 0, 0, 0]


# ---- 1. the object bank -----------------------------------------------------------------------------------------------------------
MAP = np.array([[1, 1, 0, 0, 2, 2, 2, 2, 2, 0],
                [1, 0, 0, 0, 2, 0, 0, 0, 2, 0],
                [0, 0, 0, 0, 2, 0, 1, 0, 2, 0],
                [0, 0, 0, 0, 2, 0, 0, 0, 2, 0],
                [0, 0, 0, 0, 2, 2, 2, 2, 2, 0],
                [1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                [0, 0, 2, 2, 2, 2, 2, 2, 2, 0],
                [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
RING = (MAP == 2) & (np.arange(8)[:, None] < 5)


def test_object_bank_numbers_objects_by_root_and_a_ring_keeps_its_hole():
    """Five objects of classes 1 and 2: the corner, the ring, the pixel in the ring's hole, the lone pixel, the bar - in the order of
    their first pixel.  The hole's pixel is an object of its own inside the ring's bounding box."""
    inst, bank = scenes.host_object_bank([MAP], 3, [1, 2])
    want = np.full(MAP.shape, -1, np.int32)
    want[0, 0:2] = want[1, 0] = 0
    want[RING] = 1
    want[2, 6] = 2
    want[5, 0] = 3
    want[6, 2:9] = 4
    assert inst[0].dtype == np.int32 and np.array_equal(inst[0], want)
    assert bank.dtype == np.int32 and bank.tolist() == [[0, 0, 1, 3, 0, 0, 1, 1], [0, 1, 2, 16, 0, 4, 4, 8], [0, 2, 1, 1, 2, 6, 2, 6],
                                                        [0, 3, 1, 1, 5, 0, 5, 0], [0, 4, 2, 7, 6, 2, 6, 8]]
    inst1, bank1 = scenes.host_object_bank([MAP], 3, [1])                       # the other class is no object at all
    assert sorted(set(inst1[0].ravel().tolist())) == [-1, 0, 1, 2] and bank1[:, 2].tolist() == [1, 1, 1]


def test_object_bank_filters_by_area_and_extent():
    """min_area renumbers (the ids are those of the id map), max_area and max_extent only shorten the bank."""
    inst, bank = scenes.host_object_bank([MAP, MAP.T.copy()], 3, [1, 2], min_area=2)
    assert sorted(set(inst[0].ravel().tolist())) == [-1, 0, 1, 2] and inst[0][2, 6] == -1 and inst[0][6, 5] == 2
    assert bank[:, :4].tolist() == [[0, 0, 1, 3], [0, 1, 2, 16], [0, 2, 2, 7], [1, 0, 1, 3], [1, 1, 2, 7], [1, 2, 2, 16]]
    _, small = scenes.host_object_bank([MAP], 3, [1, 2], min_area=2, max_area=10)
    assert small[:, 1].tolist() == [0, 2]
    _, narrow = scenes.host_object_bank([MAP], 3, [1, 2], min_area=2, max_extent=5)
    assert narrow[:, 1].tolist() == [0, 1]
    _, tiny = scenes.host_object_bank([MAP], 3, [1, 2], max_extent=1)
    assert tiny[:, 1].tolist() == [2, 3]
    for kw in ({"min_area": 0}, {"max_area": 1, "min_area": 2}, {"max_extent": 513}, {"max_extent": 0}):
        with pytest.raises(ValueError, match="object bank"):
            scenes.host_object_bank([MAP], 3, [1, 2], **kw)


def test_pool_object_bank_on_a_cpu_pool_and_with_paste_before_it():
    img = np.zeros(MAP.shape + (3,), np.uint8)
    pool = scenes.ScenePool([img], [MAP], patch=4, device="cpu")
    batch = pool.batch(np.array([[0, 0, 0, 0]], np.int32))
    with pytest.raises(ValueError, match="no object bank"):
        batch.with_paste(np.zeros((0, 16), np.int32))
    with pytest.raises(ValueError, match="no object bank"):
        scenes.SceneLoader(pool, np.array([[0, 0, 0, 0]], np.int32), 1, paste=scenes.CopyPaste([1]))
    bank = pool.object_bank(3, [1, 2])                                          # max_extent: the patch side, 4
    assert bank is pool.bank and bank[:, 1].tolist() == [0, 2, 3] and pool.bank_classes == 3
    assert np.array_equal(pool.inst_maps[0], scenes.host_object_bank([MAP], 3, [1, 2])[0][0])
    assert batch.with_paste(np.zeros((0, 16), np.int32)).paste.shape == (0, 16)


# ---- 2. host_paste against hand-written answers ------------------------------------------------------------------------------------
# a 2 x 3 crop at (1, 2) of a 4 x 6 scene: the L-shaped object 7 is the pixels valued 1, 2, 3, 4; the pixel valued 5 belongs to
# object 8 of the same class, INSIDE the L's bounding box; the pixel valued 6 is background
S_IMG = np.array([[90, 91, 92, 93, 94, 95], [96, 97, 1, 2, 3, 98], [99, 89, 4, 5, 6, 88], [87, 86, 85, 84, 83, 82]], np.uint8)
S_CLS = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 2, 2, 2, 0], [0, 0, 2, 2, 1, 0], [0, 0, 0, 0, 0, 0]], np.uint8)
S_INST = np.array([[-1] * 6, [-1, -1, 7, 7, 7, -1], [-1, -1, 7, 8, -1, -1], [-1] * 6], np.int32)
# what each code leaves of the L (0: the window keeps its byte), written out by hand from the table of codes in scenes.py
L_UNDER = {0: [[1, 2, 3], [4, 0, 0]], 1: [[3, 0], [2, 0], [1, 4]], 2: [[0, 0, 4], [3, 2, 1]], 3: [[4, 0, 0], [1, 2, 3]],
           4: [[3, 2, 1], [0, 0, 4]], 5: [[4, 1], [0, 2], [0, 3]], 6: [[1, 4], [2, 0], [3, 0]], 7: [[0, 3], [0, 2], [4, 1]]}


def scene3(cin):
    """The scene above with `cin` channels: channel c of a pixel valued v holds v + 100 c (mod 256)."""
    return (S_IMG[..., None].astype(np.int64) + 100 * np.arange(cin)).astype(np.uint8)


def paste_L(PH, PW, rows, cin=2, cls0=0, C=3):
    """host_paste of `rows` into windows whose image bytes are 200 and whose class bytes are cls0: (img, cls, img before, cls
    before).  The arguments must come back unchanged; whether the result differs from them is the caller's to assert."""
    N = 1 + max([r[0] for r in rows], default=0)
    img0 = np.full((N, PH, PW, cin), 200, np.uint8)
    c0 = np.broadcast_to(np.asarray(cls0, np.uint8), (N, PH, PW)).copy()
    img, cls = scenes.host_paste(img0, c0, [scene3(cin)], [S_CLS], [S_INST], np.array(rows, np.int64).reshape(-1, 16), C)
    assert img0.min() == 200 == img0.max() and np.array_equal(c0, np.broadcast_to(np.asarray(cls0, np.uint8), (N, PH, PW))), "the arguments changed"
    return img, cls, img0, c0


def expect(PH, PW, placed, top, left, cin=2):
    """Windows of 200s / class 0 with the hand-written value array `placed` at (top, left), clipped; 0 keeps the window's byte."""
    img = np.full((PH, PW, cin), 200, np.uint8)
    cls = np.zeros((PH, PW), np.uint8)
    for u, line in enumerate(placed):
        for v, val in enumerate(line):
            y, x = top + u, left + v
            if val and 0 <= y < PH and 0 <= x < PW:
                img[y, x] = [(val + 100 * c) % 256 for c in range(cin)]
                cls[y, x] = 2
    return img, cls


@pytest.mark.parametrize("code", range(8))
def test_L_shaped_object_under_every_code(code):
    """A non-square crop under each of the eight symmetries, in a non-square window; the neighbour with another id and the
    background inside the bounding box stay out."""
    img, cls, img0, cls0 = paste_L(5, 6, [row(0, 0, 7, code, 1, 2, 1, 2, 2, 3)])
    want_img, want_cls = expect(5, 6, L_UNDER[code], 1, 2)
    assert np.array_equal(img[0], want_img) and np.array_equal(cls[0], want_cls)
    assert not np.array_equal(img, img0) and not np.array_equal(cls, cls0)
    assert (cls[0] == 2).sum() == 4


@pytest.mark.parametrize("top,left,kept", [(-1, 1, [4]), (3, 1, [1, 2, 3]), (1, -1, [2, 3]), (1, 3, [1, 2, 4]), (-1, -2, []), (3, 4, [1])])
def test_clipping_at_each_window_edge(top, left, kept):
    """Code 0 in a 4 x 5 window: over the top edge only the L's foot is left, over the bottom edge its bar, over the left edge the
    bar's end, over the right edge all but the bar's end; a corner keeps one pixel or none."""
    img, cls, img0, cls0 = paste_L(4, 5, [row(0, 0, 7, 0, top, left, 1, 2, 2, 3)])
    want_img, want_cls = expect(4, 5, L_UNDER[0], top, left)
    assert np.array_equal(img[0], want_img) and np.array_equal(cls[0], want_cls)
    assert sorted(int(v) for v in img[0][..., 0][cls[0] == 2]) == kept
    assert np.array_equal(img, img0) == (not kept)


def test_rows_wholly_outside_are_no_ops_and_other_windows_keep_their_bits():
    outside = [row(0, 0, 7, 0, 4, 0, 1, 2, 2, 3), row(0, 0, 7, 0, 0, 5, 1, 2, 2, 3), row(0, 0, 7, 0, -2, 0, 1, 2, 2, 3), row(0, 0, 7, 1, 0, -2, 1, 2, 2, 3),
               row(0, 0, 7, 0, 1024, -1024, 1, 2, 2, 3)]
    img, cls, img0, cls0 = paste_L(4, 5, outside)
    assert np.array_equal(img, img0) and np.array_equal(cls, cls0)
    img, cls, img0, cls0 = paste_L(4, 5, [row(0, 0, 9, 0, 0, 0, 1, 2, 2, 3)])                       # an id no pixel carries
    assert np.array_equal(img, img0) and np.array_equal(cls, cls0)
    img, cls, img0, cls0 = paste_L(4, 5, [row(0, 0, 7, 0, 0, 0, 1, 2, 2, 3), row(2, 0, 7, 0, 1, 1, 1, 2, 2, 3)])
    assert np.array_equal(img[1], img0[1]) and np.array_equal(cls[1], cls0[1])
    assert not np.array_equal(img[0], img0[0]) and not np.array_equal(img[2], img0[2])
    img, cls, img0, cls0 = paste_L(4, 5, [])
    assert np.array_equal(img, img0) and np.array_equal(cls, cls0)


def test_three_overlapping_rows_the_last_wins_and_onto_sees_earlier_pastes():
    """Three 1 x 3 bars of classes 1, 2, 3 into a 1 x 5 window of class 0: the second may cover class 0 only and so loses the two
    pixels the first took; the third may cover classes 1 and 2 and so takes one pixel of each and leaves the last, still class 0."""
    s_img = np.arange(10, 28, dtype=np.uint8).reshape(3, 6, 1)
    s_cls = np.repeat(np.array([[1], [2], [3]], np.uint8), 6, 1)
    s_inst = np.repeat(np.array([[0], [1], [2]], np.int32), 6, 1)
    img0, cls0 = np.full((1, 1, 5, 1), 200, np.uint8), np.zeros((1, 1, 5), np.uint8)
    rows = [row(0, 0, 0, 0, 0, 0, 0, 0, 1, 3, lo=1, hi=0), row(0, 0, 1, 0, 0, 1, 1, 0, 1, 3, lo=1, hi=0), row(0, 0, 2, 0, 0, 2, 2, 0, 1, 3, lo=6, hi=0)]
    img, cls = scenes.host_paste(img0, cls0, [s_img], [s_cls], [s_inst], rows, 4)
    assert cls[0, 0].tolist() == [1, 1, 3, 3, 0] and img[0, 0, :, 0].tolist() == [10, 11, 22, 23, 200]
    img, cls = scenes.host_paste(img0, cls0, [s_img], [s_cls], [s_inst], rows[:2], 4)
    assert cls[0, 0].tolist() == [1, 1, 1, 2, 0] and img[0, 0, :, 0].tolist() == [10, 11, 12, 18, 200]
    img, cls = scenes.host_paste(img0, cls0, [s_img], [s_cls], [s_inst], rows[1:2], 4)                # without the first row it takes all three
    assert cls[0, 0].tolist() == [0, 2, 2, 2, 0]
    hi = scenes.host_paste(img0, np.full((1, 1, 5), 40, np.uint8), [s_img], [s_cls], [s_inst], [row(0, 0, 0, 0, 0, 0, 0, 0, 1, 3, lo=0, hi=1 << 8)], 64)
    assert hi[1][0, 0].tolist() == [1, 1, 1, 40, 40]                                                 # bit 40 lives in the high word


def test_over_void_on_and_off():
    """Destination bytes >= num_classes hold no class: bit d of onto says nothing about them, only the flag does."""
    void = np.array([[0, 255, 3, 0, 0], [0, 3, 0, 0, 0], [0] * 5, [0] * 5], np.uint8)                # 3 == num_classes is void too
    off = paste_L(4, 5, [row(0, 0, 7, 0, 0, 0, 1, 2, 2, 3, flags=0)], cls0=void)
    assert off[1][0].tolist() == [[2, 255, 3, 0, 0], [2, 3, 0, 0, 0], [0] * 5, [0] * 5] and not np.array_equal(off[1], off[3])
    on = paste_L(4, 5, [row(0, 0, 7, 0, 0, 0, 1, 2, 2, 3, flags=1)], cls0=void)
    assert on[1][0].tolist() == [[2, 2, 2, 0, 0], [2, 3, 0, 0, 0], [0] * 5, [0] * 5]
    only = paste_L(4, 5, [row(0, 0, 7, 0, 0, 0, 1, 2, 2, 3, lo=0, hi=0, flags=1)], cls0=void)
    assert only[1][0].tolist() == [[0, 2, 2, 0, 0], [0, 3, 0, 0, 0], [0] * 5, [0] * 5] and only[0][0, 0, 1].tolist() == [2, 102]
    none = paste_L(4, 5, [row(0, 0, 7, 0, 0, 0, 1, 2, 2, 3, lo=0, hi=0, flags=0)], cls0=void)
    assert np.array_equal(none[0], none[2]) and np.array_equal(none[1], none[3])


# ---- 3. check_paste_table ----------------------------------------------------------------------------------------------------------
GOOD = row(1, 0, 7, 3, -2, 4, 1, 2, 2, 3)
BAD_WORDS = [(0, 2, "row 1: word 0: window 2 outside 0..1"), (0, -1, "row 1: word 0: window -1 outside 0..1"),
             (0, 0, r"row 1: word 0: window 0 after window 1 \(rows are sorted by window\)"),
             (1, 1, "row 1: word 1: scene 1 outside 0..0"), (1, -1, "row 1: word 1: scene -1 outside 0..0"), (2, -1, "row 1: word 2: id -1 is negative"),
             (3, 8, "row 1: word 3: code 8 outside 0..7"), (3, -1, "row 1: word 3: code -1 outside 0..7"),
             (4, 1025, "row 1: word 4: top 1025 outside -1024..1024"), (5, -1025, "row 1: word 5: left -1025 outside -1024..1024"),
             (6, 3, "row 1: word 6: rows 3 \\+ 2 leave the 4 x 6 scene"), (6, -1, "row 1: word 6: rows -1 \\+ 2 leave"),
             (7, 4, "row 1: word 7: columns 4 \\+ 3 leave the 4 x 6 scene"), (7, -1, "row 1: word 7: columns -1 \\+ 3 leave"),
             (8, 0, "row 1: word 8: h 0 outside 1..512"), (8, 513, "row 1: word 8: h 513 outside 1..512"),
             (9, 0, "row 1: word 9: w 0 outside 1..512"), (9, 513, "row 1: word 9: w 513 outside 1..512"),
             (12, 2, "row 1: word 12: flags 2"), (12, -1, "row 1: word 12: flags -1"),
             (13, 1, "row 1: word 13: reserved, must be 0, got 1"), (14, -5, "row 1: word 14: reserved, must be 0, got -5"),
             (15, 9, "row 1: word 15: reserved, must be 0, got 9")]


def bad_table(word, value):
    t = np.array([GOOD, GOOD], np.int64)
    t[1, word] = value
    return t


@pytest.mark.parametrize("word,value,message", BAD_WORDS)
def test_check_paste_table_refuses_each_word(word, value, message):
    assert scenes.check_paste_table([(4, 6)], [GOOD, GOOD], 2, (4, 5), 3).dtype == np.int32
    with pytest.raises(ValueError, match="rua_window_paste: " + message):
        scenes.check_paste_table([(4, 6)], bad_table(word, value), 2, (4, 5), 3)
    with pytest.raises(ValueError, match="rua_window_paste: " + message):
        scenes.host_paste(np.zeros((2, 4, 5, 1), np.uint8), np.zeros((2, 4, 5), np.uint8), [S_IMG[..., None]], [S_CLS], [S_INST], bad_table(word, value), 3)


def test_check_paste_table_refuses_the_call_arguments():
    ok = np.array([GOOD], np.int64)
    ok[0, 0] = 0
    for kw, message in (({"N": 0}, r"N 0 \(>= 1\)"), ({"patch": (0, 5)}, "PH 0, PW 5"), ({"patch": (4, 513)}, "PH 4, PW 513"), ({"num_classes": 0}, "C 0 outside 1..64"),
                        ({"num_classes": 65}, "C 65 outside 1..64"), ({"channels": 17}, "Cin 17 outside 1..16"), ({"N": 512, "patch": 512, "channels": 16}, r"N\*PH\*PW\*Cin is 2147483648 \(must stay below 2\^31\)")):
        args = dict({"N": 1, "patch": (4, 5), "num_classes": 3, "channels": 1}, **kw)
        with pytest.raises(ValueError, match="rua_window_paste: " + message):
            scenes.check_paste_table([(4, 6)], ok, args["N"], args["patch"], args["num_classes"], args["channels"])
    for t in (np.zeros((2, 15), np.int32), np.zeros((2, 16), np.float32), np.zeros(16, np.int32)):
        with pytest.raises(ValueError, match="a paste table is an integer"):
            scenes.check_paste_table([(4, 6)], t, 1, (4, 5), 3)
    assert scenes.check_paste_table([(4, 6)], np.zeros((0, 16), np.int32), 1, (4, 5), 3).shape == (0, 16)
    both = scenes.check_paste_table([(4, 6)], [row(0, 0, 1, 0, 0, 0, 0, 0, 1, 1, lo=0xFFFFFFFF, hi=1 << 31)], 1, (4, 5), 3)
    assert both[0, 10] == -1 and both[0, 11] == -(1 << 31)                       # the mask words are taken mod 2^32


# ---- 4. paste_rows and CopyPaste ---------------------------------------------------------------------------------------------------
def test_paste_rows_from_bank_entries():
    _, bank = scenes.host_object_bank([MAP], 3, [1, 2])
    t = scenes.paste_rows(bank, [0, 0, 2], [1, 4, 0], [0, 6, 3], [5, -1, 0], 7, onto={2: [0, 1]}, over_void=True)
    assert t.dtype == np.int32 and t.tolist() == [row(0, 0, 1, 0, 5, 7, 0, 4, 5, 5, lo=3, hi=0, flags=1), row(0, 0, 4, 6, -1, 7, 6, 2, 1, 7, lo=3, hi=0, flags=1),
                                                  row(2, 0, 0, 3, 0, 7, 0, 0, 2, 2, lo=ALL, hi=ALL, flags=1)]
    assert scenes.paste_rows(bank, 0, 1, 0, 0, 0, onto=[2])[0, 10:13].tolist() == [4, 0, 0]
    assert scenes.paste_rows(bank, 0, 1, 0, 0, 0, onto=[40])[0, 10:12].tolist() == [0, 256]
    with pytest.raises(ValueError, match="bank_index"):
        scenes.paste_rows(bank, 0, 5, 0, 0, 0)


def long_tailed_bank():
    """100 objects of class 1, two of class 3 and one of class 2 in two scenes, of sizes up to 9 x 12; one class-3 giant of 40 x 8."""
    rng = np.random.default_rng(5)
    rows = []
    for k in range(104):
        c = 1 if k < 100 else 2 if k == 100 else 3
        h, w = (40, 8) if k == 103 else (int(rng.integers(1, 10)), int(rng.integers(1, 13)))
        i, j = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        rows.append([k % 2, k // 2, c, h * w, i, j, i + h - 1, j + w - 1])
    return np.array(rows, np.int32)


def test_copy_paste_draw_is_seeded_sorted_and_inside():
    bank = long_tailed_bank()
    cp = scenes.CopyPaste([1, 3], per_window=(0, 3), onto={3: [0]}, over_void=True)
    t = cp.draw(np.random.default_rng([3, 0, 1, 2]), bank, 400, (20, 16), 4)
    assert np.array_equal(t, cp.draw(np.random.default_rng([3, 0, 1, 2]), bank, 400, (20, 16), 4))
    assert not np.array_equal(t, cp.draw(np.random.default_rng([3, 0, 2, 2]), bank, 400, (20, 16), 4))
    assert t.dtype == np.int32 and t.shape[1] == 16 and (np.diff(t[:, 0]) >= 0).all()
    per = np.bincount(t[:, 0], minlength=400)
    assert per.min() == 0 and per.max() == 3 and set(per.tolist()) == {0, 1, 2, 3}
    scenes.check_paste_table([(70, 70), (70, 70)], t, 400, (20, 16), 4)
    tr = np.isin(t[:, 3], scenes.TRANSPOSING)
    th, tw = np.where(tr, t[:, 9], t[:, 8]), np.where(tr, t[:, 8], t[:, 9])
    assert (t[:, 4] >= 0).all() and (t[:, 5] >= 0).all() and (t[:, 4] + th <= 20).all() and (t[:, 5] + tw <= 16).all()
    assert set(t[:, 3].tolist()) == set(range(8)) and (t[:, 4] + th == 20).any() and (t[:, 4] == 0).any()
    key = {(int(b[0]), int(b[1])): b for b in bank}
    for r in t:
        b = key[(int(r[1]), int(r[2]))]
        assert b[2] in (1, 3) and r[6:10].tolist() == [b[4], b[5], b[6] - b[4] + 1, b[7] - b[5] + 1] and max(r[8], r[9]) <= 16      # never the giant
        assert r[10:13].tolist() == ([1, 0, 1] if b[2] == 3 else [ALL, ALL, 1])


def test_copy_paste_draws_classes_uniformly_not_objects():
    """100 objects of class 1 against one drawable object of class 3: half of the pastes are that one object (M = 6000 pastes, the
    share's standard deviation is 0.0065: 0.45..0.55 is more than seven of them)."""
    bank = long_tailed_bank()
    t = scenes.CopyPaste([1, 3], per_window=(3, 3)).draw(np.random.default_rng(0), bank, 2000, 64, 4)
    cls_of = {(int(b[0]), int(b[1])): int(b[2]) for b in bank}
    drawn = np.array([cls_of[(int(r[1]), int(r[2]))] for r in t])
    assert len(t) == 6000 and 0.45 < (drawn == 3).mean() < 0.55 and set(drawn.tolist()) == {1, 3}
    ones = np.bincount(t[drawn == 1, 2] * 2 + t[drawn == 1, 1], minlength=100)
    assert (ones > 0).all()                                                     # every object of the common class turns up
    assert len(scenes.CopyPaste([0]).draw(np.random.default_rng(0), bank, 50, 64, 4)) == 0           # a class without objects
    assert len(scenes.CopyPaste([1], per_window=(0, 0)).draw(np.random.default_rng(0), bank, 50, 64, 4)) == 0
    for kw in ({"classes": []}, {"classes": [64]}, {"classes": [1], "per_window": (2, 1)}, {"classes": [1], "per_window": (-1, 1)}):
        with pytest.raises(ValueError):
            scenes.CopyPaste(**kw)
    with pytest.raises(ValueError, match="for a model of 3 classes"):
        scenes.CopyPaste([1, 3]).draw(np.random.default_rng(0), bank, 5, 64, 3)


# ---- 5. batches and the loader -----------------------------------------------------------------------------------------------------
def blob_cpu_pool():
    rng = np.random.default_rng(9)
    cls = [np.kron(rng.integers(0, 4, (12, 14)), np.ones((8, 8), np.int64)).astype(np.uint8) for _ in range(2)]
    img = [rng.integers(0, 256, c.shape + (3,)).astype(np.uint8) for c in cls]
    pool = scenes.ScenePool(img, cls, patch=32, device="cpu")
    pool.object_bank(4, [1, 3])
    return pool


@pytest.fixture(scope="module")
def pool():
    return blob_cpu_pool()


def test_scene_batch_slicing_renumbers_windows_and_host_is_cut_paste_photo(pool):
    rows4 = np.array([[0, 3, 5, 0], [1, 20, 40, 2], [0, 60, 70, 3], [1, 0, 0, 4]], np.int32)
    table = scenes.CopyPaste([1, 3], per_window=(1, 3)).draw(np.random.default_rng(4), pool.bank, 4, 32, 4)
    photo = scenes.PhotoJitter().draw(np.random.default_rng(5), 4, 3)
    for batch in (pool.batch(rows4), pool.affine_batch(scenes.affine_rows(rows4, 32, [10.0, -30.0, 80.0, 5.0], [1.0, 1.3, 0.8, 1.0]))):
        b = batch.with_paste(table).with_photo(photo)
        assert type(b) is type(batch) and b.paste is not table and np.array_equal(b.paste, table) and np.array_equal(b.photo, photo)
        assert b.with_photo(None).paste is b.paste and b.with_paste(None).photo is b.photo and b.with_paste(None).paste is None
        cut = batch.host()
        pasted = scenes.host_paste(cut[0], cut[1], pool.images, pool.class_maps, pool.inst_maps, table, 4)
        assert not np.array_equal(pasted[0], cut[0]) and not np.array_equal(pasted[1], cut[1])
        got = b.host()
        assert np.array_equal(got[0], scenes.host_photometric(pasted[0], photo)) and np.array_equal(got[1], pasted[1])
        part = b[1:3]
        assert part.paste[:, 0].tolist() == (table[(table[:, 0] >= 1) & (table[:, 0] < 3), 0] - 1).tolist()
        assert np.array_equal(part.paste[:, 1:], table[(table[:, 0] >= 1) & (table[:, 0] < 3), 1:])
        for k, sl in enumerate((slice(0, 2), slice(2, 4))):
            half = b.shard(k, 2)
            assert np.array_equal(half.paste, b[sl].paste) and set(half.paste[:, 0].tolist()) <= {0, 1}
            assert np.array_equal(half.host()[0], got[0][sl]) and np.array_equal(half.host()[1], got[1][sl])
        assert b[3:].paste[:, 0].tolist() == [0] * int((table[:, 0] == 3).sum())
    with pytest.raises(ValueError, match="row 0: word 0: window 4 outside 0..3"):
        pool.batch(rows4).with_paste(scenes.paste_rows(pool.bank, 4, 0, 0, 0, 0))


def loader_batches(pool, rank, world, **kw):
    table = scenes.window_table(pool.shapes, 32, 16, False)
    ld = scenes.SceneLoader(pool, table, 4, rank=rank, world=world, order=np.arange(16), seed=11, **kw)
    return [[b for b, _ in ld] for _ in range(2)]                               # two passes


def test_loader_world_of_two_sees_what_a_world_of_one_sees_and_other_draws_stay(pool):
    paste = scenes.CopyPaste([1, 3], per_window=(1, 3))
    jit, pho = scenes.Jitter(shift=4.0), scenes.PhotoJitter()
    for kw in ({}, {"jitter": jit}, {"photo": pho}, {"jitter": jit, "photo": pho}):
        one = loader_batches(pool, 0, 1, paste=paste, **kw)
        two = [loader_batches(pool, r, 2, paste=paste, **kw) for r in (0, 1)]
        plain = loader_batches(pool, 0, 1, **kw)
        tables = []
        for e in range(2):
            for k in range(4):
                g = one[e][k]
                assert g.paste is not None and len(g.paste) >= 4
                want = paste.draw(np.random.default_rng([11, e, k, 2]), pool.bank, 4, 32, 4)
                assert np.array_equal(g.paste, want)
                tables.append(want.tobytes())
                halves = [two[r][e][k] for r in (0, 1)]
                assert all(len(h) == 2 for h in halves)
                joined = np.concatenate([halves[0].paste, halves[1].paste + np.eye(16, dtype=np.int32)[0] * 2])
                assert np.array_equal(joined, g.paste)
                for r in (0, 1):
                    assert np.array_equal(halves[r].host()[0], g.host()[0][2 * r:2 * r + 2]) and np.array_equal(halves[r].host()[1], g.host()[1][2 * r:2 * r + 2])
                p = plain[e][k]                                                 # jitter= and photo= draw what they drew without paste=
                assert p.paste is None and type(p) is type(g) and np.array_equal(p.rows, g.rows)
                assert (p.photo is None) == (g.photo is None) and (p.photo is None or np.array_equal(p.photo, g.photo))
        assert len(set(tables)) == 8                                            # every batch of every pass draws afresh
