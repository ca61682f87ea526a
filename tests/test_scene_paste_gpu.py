"""GPU tests of the copy-paste augmentation: rua_window_paste (csrc/paste.hip) bit for bit against scenes.host_paste; the engine's
buffers after _upload_scene with a paste table against _upload_compact fed with batch.host(), and the calls a batch issues with and
without a table; training steps over the scene route against the compact route on the same bytes; ScenePool.object_bank on the GPU
against scenes.host_object_bank; the CLI with --paste_aug yes."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

from _scene_util import GUARD, HEADS, NCLS as C, SHAPE, blob_scene, new_engine, new_training_model, read_scalars, state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [1, 3]                                             # the classes whose regions are objects
with open(os.path.join(ROOT, "resunet_a_mltsk_keras_amd", "csrc", "paste.hip")) as f:
    PER_LAUNCH = int(re.search(r"constexpr int PA_CHUNK = (\d+);", f.read()).group(1))


# ---- 1. the kernel against its numpy definition -----------------------------------------------------------------------------------
class Scenes:
    """Two scenes of 150 x 171 and 131 x 160 with 16 image channels (a test takes the first Cin), blob class maps with hand-placed
    objects in the first - each with a margin of class 0 around it, so it is an object of its own - and the id maps and bank of
    host_object_bank.  `at` names the hand-placed ones by their bank row."""

    def __init__(self):
        rng = np.random.default_rng(77)
        cls = [blob_scene(300)[1], blob_scene(301, 131, 160)[1]]
        c0 = cls[0]
        c0[20:23, 20:23], c0[21, 21] = 0, 3                                    # one pixel
        c0[50:92, 60:107], c0[51:91, 61:106], c0[60:70, 70:80] = 0, 1, 2       # 40 x 45 with a hole of another class
        c0[0:4, 99:110], c0[0:3, 100:109] = 0, 3                               # 3 x 9, touches scene row 0
        c0[99:106, 163:171], c0[100:105, 164:171] = 0, 1                       # 5 x 7, touches the last column
        c0[120:124, 10:40] = 255                                               # a stripe that holds no class
        self.cls = cls
        self.img16 = [rng.integers(0, 256, c.shape + (16,)).astype(np.uint8) for c in cls]
        self.inst, self.bank = scenes.host_object_bank(cls, C, CLASSES)
        row_of = {(int(b[0]), int(b[1])): k for k, b in enumerate(self.bank)}
        self.at = {name: row_of[(0, int(self.inst[0][p]))] for name, p in (("pixel", (21, 21)), ("big", (51, 61)), ("top", (0, 100)), ("right", (100, 170)))}
        for name, hw in (("pixel", (1, 1)), ("big", (40, 45)), ("top", (3, 9)), ("right", (5, 7))):
            b = self.bank[self.at[name]]
            assert (b[6] - b[4] + 1, b[7] - b[5] + 1) == hw, (name, b.tolist())
        assert self.bank[self.at["top"], 4] == 0 and self.bank[self.at["right"], 7] == 170
        self.dev = None

    def images(self, cin):
        return [np.ascontiguousarray(a[..., :cin]) for a in self.img16]

    def device(self, cin):
        """(keep-alive list, img pointers, cls pointers, inst pointers, heights, widths) of the scenes with cin channels."""
        t = [[torch.from_numpy(a).cuda() for a in arrs] for arrs in (self.images(cin), self.cls, self.inst)]
        ptrs = [(ctypes.c_void_p * 2)(*[x.data_ptr() for x in part]) for part in t]
        hs, ws = (ctypes.c_int32 * 2)(*[c.shape[0] for c in self.cls]), (ctypes.c_int32 * 2)(*[c.shape[1] for c in self.cls])
        return t, ptrs[0], ptrs[1], ptrs[2], hs, ws


@pytest.fixture(scope="module")
def scn():
    return Scenes()


def run_paste(scn, img, cls, table, num_classes=C):
    """rua_window_paste on device copies of img and cls; GUARD bytes behind either must come back untouched."""
    N, PH, PW, Cin = img.shape
    bufs = []
    for a, fill in ((img, 0x5A), (cls, 0xA5)):
        b = torch.full((a.size + GUARD,), fill, dtype=torch.uint8, device="cuda")
        b[:a.size] = torch.from_numpy(a.ravel()).cuda()
        bufs.append(b)
    keep, ip, cp, np_, hs, ws = scn.device(Cin)
    t = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 16)
    L.lib().call("rua_window_paste", bufs[0].data_ptr(), bufs[1].data_ptr(), N, PH, PW, Cin, num_classes, ip, cp, np_, hs, ws, 2,
                 t.ctypes.data if len(t) else None, len(t), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    gi, gc = bufs[0].cpu().numpy(), bufs[1].cpu().numpy()
    assert (gi[img.size:] == 0x5A).all(), "bytes behind img were written"
    assert (gc[cls.size:] == 0xA5).all(), "bytes behind cls were written"
    return gi[:img.size].reshape(img.shape), gc[:cls.size].reshape(cls.shape)


def windows(rng, PH, PW, N, Cin):
    """Random image bytes; class bytes 0..3 with two kinds of void (4, the first value that is no class, and 255)."""
    img = rng.integers(0, 256, (N, PH, PW, Cin)).astype(np.uint8)
    cls = rng.choice(np.array([0, 1, 2, 3, 4, 255], np.uint8), (N, PH, PW), p=[0.3, 0.2, 0.2, 0.1, 0.1, 0.1])
    return img, cls


def kernel_rows(rng, scn, PH, PW, N):
    """The rows of one bitwise case, sorted by window; window 1 gets none.
    window 0: the pixel, the 3 x 9 (scene row 0) and the 5 x 7 (last scene column) objects under all eight codes at places that clip
              at the top, the bottom, the left and the right edge and in the middle, every destination class allowed, void too;
              then a stack three deep whose masks refer to the classes the rows below leave;
    window 2: (and every further one but the last) random objects, codes, places half outside, masks and flags;
    last:     the 40 x 45 object at (10, 12) - over the tile seams of a 64 x 64 window - under four codes on top of one another,
              then random rows."""
    at, bank = scn.at, scn.bank
    rows = []
    add = lambda w, k, code, top, left, mask, over: rows.append(scenes.paste_rows(bank, w, k, code, top, left, onto=mask, over_void=over)[0])
    every, n = list(range(C)), 0
    for name in ("pixel", "top", "right") * (PER_LAUNCH // 24 + 1):          # more rows than one launch holds: they straddle launches
        b = bank[at[name]]
        h, w = int(b[6] - b[4] + 1), int(b[7] - b[5] + 1)
        for code in range(8):
            th, tw = (w, h) if code in scenes.TRANSPOSING else (h, w)
            places = [(-(th // 2), 1), (PH - (th + 1) // 2, 0), (1, -(tw // 2)), (0, PW - (tw + 1) // 2), ((PH - th) // 2, (PW - tw) // 2)]
            top, left = places[n % 5]
            n += 1
            add(0, at[name], code, top, left, every, True)
    add(0, at["right"], 0, 0, 0, every, True)                                   # class 1 ...
    add(0, at["top"], 6, 0, 0, [1], False)                                      # ... class 3 only where the row below pasted
    add(0, at["right"], 4, 1, 1, [3, 0], False)                                 # ... class 1 over that and over class 0, never over void
    small = np.flatnonzero(np.maximum(bank[:, 6] - bank[:, 4], bank[:, 7] - bank[:, 5]) < 64)

    def random_rows(w, count):
        for _ in range(count):
            k = int(rng.choice(small))
            h, wd = int(bank[k, 6] - bank[k, 4] + 1), int(bank[k, 7] - bank[k, 5] + 1)
            mask = [c for c in range(C) if rng.random() < 0.6]
            add(w, k, int(rng.integers(0, 8)), int(rng.integers(-max(h, wd) + 1, PH)), int(rng.integers(-max(h, wd) + 1, PW)), mask, bool(rng.integers(0, 2)))

    for w in range(2, N - 1):
        random_rows(w, 12)
    for code, mask, over in ((0, every, True), (5, [0, 2], False), (2, [1], True), (7, [], True)):
        add(N - 1, at["big"], code, 10, 12, mask, over)
    random_rows(N - 1, 10)
    return np.array(rows, np.int32)


@pytest.mark.parametrize("PH,PW,N,Cin", [(5, 7, 3, 3), (33, 31, 4, 1), (9, 9, 3, 7), (1, 1, 5, 16), (64, 64, 4, 3)])
def test_paste_bitwise(scn, PH, PW, N, Cin):
    """Odd windows, one channel and seven and sixteen, one-pixel windows, and 64 x 64 ones of four tiles.  Window 0 alone holds more
    rows than one launch, so its rows straddle launches; window 1 has none and keeps its bits."""
    rng = np.random.default_rng(PH * 131 + PW * 7 + N + Cin)
    img, cls = windows(rng, PH, PW, N, Cin)
    table = kernel_rows(rng, scn, PH, PW, N)
    assert (table[:, 0] == 0).sum() > PER_LAUNCH and (table[:, 0] == 1).sum() == 0 and (np.diff(table[:, 0]) >= 0).all()
    assert set(table[:, 3].tolist()) == set(range(8)) and {0, 1} == set(table[:, 12].tolist())
    want_img, want_cls = scenes.host_paste(img, cls, scn.images(Cin), scn.cls, scn.inst, table, C)
    assert not np.array_equal(want_img, img) and not np.array_equal(want_cls, cls)
    got_img, got_cls = run_paste(scn, img, cls, table)
    for got, want, what in ((got_cls, want_cls, "cls"), (got_img, want_img, "img")):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, len(bad), "first at", tuple(bad[0]))
    assert np.array_equal(got_img[1], img[1]) and np.array_equal(got_cls[1], cls[1])
    if (PH, PW) == (64, 64):                                                    # the big object really lies over all four tiles
        changed = got_cls[N - 1] != cls[N - 1]
        assert changed[:32, :32].any() and changed[:32, 32:].any() and changed[32:, :32].any() and changed[32:, 32:].any()
    none_img, none_cls = run_paste(scn, img, cls, np.zeros((0, 16), np.int32))  # M == 0
    assert np.array_equal(none_img, img) and np.array_equal(none_cls, cls)


def test_paste_more_rows_than_a_launch_over_many_windows(scn):
    """70 rows (or the launch size + 22, if that is more) over 50 windows of 6 x 8; the rows with numbers PER_LAUNCH - 1 and
    PER_LAUNCH are two overlapping objects of different classes in ONE window, so that window's answer depends on the order of
    two launches."""
    M, N = max(70, PER_LAUNCH + 22), 50
    win = np.minimum(np.arange(M) * N // M, N - 1)
    win[PER_LAUNCH] = win[PER_LAUNCH - 1]
    assert (np.diff(win) >= 0).all() and len(set(win.tolist())) > 40
    k = np.where(np.arange(M) % 2 == 0, scn.at["right"], scn.at["top"])
    table = scenes.paste_rows(scn.bank, win, k, np.arange(M) % 8, np.arange(M) % 2, np.arange(M) % 3, over_void=True)
    rng = np.random.default_rng(3)
    img, cls = windows(rng, 6, 8, N, 3)
    want_img, want_cls = scenes.host_paste(img, cls, scn.images(3), scn.cls, scn.inst, table, C)
    w = int(win[PER_LAUNCH])
    swapped = table.copy()
    swapped[[PER_LAUNCH - 1, PER_LAUNCH]] = table[[PER_LAUNCH, PER_LAUNCH - 1]]
    assert not np.array_equal(scenes.host_paste(img, cls, scn.images(3), scn.cls, scn.inst, swapped, C)[1][w], want_cls[w]), "the order must matter"
    got_img, got_cls = run_paste(scn, img, cls, table)
    assert np.array_equal(got_cls, want_cls) and np.array_equal(got_img, want_img)
    assert not np.array_equal(want_img, img)


def test_paste_refuses_in_the_words_of_check_paste_table(scn):
    """One table per refused word and one call per refused argument: the library says what check_paste_table says, and the buffers
    of a refused call keep their bytes - nothing was launched."""
    good = scenes.paste_rows(scn.bank, [1, 1], scn.at["top"], 3, 1, 2)
    rng = np.random.default_rng(8)
    img, cls = windows(rng, 8, 9, 2, 3)
    shapes = [c.shape for c in scn.cls]
    cases = [(0, 2), (0, 0), (1, 2), (1, -1), (2, -1), (3, 8), (4, -1025), (5, 1025), (6, 148), (7, 163), (8, 0), (8, 513), (9, 513), (12, 2), (13, 1), (14, 1), (15, -1)]
    for word, value in cases:
        bad = good.copy()
        bad[1, word] = value
        with pytest.raises(ValueError) as host:
            scenes.check_paste_table(shapes, bad, 2, (8, 9), C, 3)
        assert f"row 1: word {word}:" in str(host.value)
        with pytest.raises(L.RuaError) as dev:
            run_paste(scn, img, cls, bad)
        assert str(dev.value).endswith(str(host.value)), (str(dev.value), str(host.value))
    for num_classes in (0, 65):
        with pytest.raises(ValueError) as host:
            scenes.check_paste_table(shapes, good, 2, (8, 9), num_classes, 3)
        with pytest.raises(L.RuaError) as dev:
            run_paste(scn, img, cls, good, num_classes)
        assert str(dev.value).endswith(str(host.value))
    got = run_paste(scn, img, cls, good)
    assert not np.array_equal(got[0], img)


# ---- 2. engine --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """Two blob scenes, the first with a stripe that holds no class, and the bank of their objects of classes 1 and 3."""
    sc = [blob_scene(100), blob_scene(101)]
    sc[0][1][40:60, 30:120] = 255
    p = scenes.ScenePool([s[0] for s in sc], [s[1] for s in sc], patch=64)
    p.object_bank(C, CLASSES, min_area=4)
    return p


def paste_batch(pool, seed, affine, photo, B=2):
    """B windows - the first over the void stripe of scene 0 -, plain (any code) or under a rotation, zoom and shift, with the table
    CopyPaste draws (objects may cover void) plus one object put onto the stripe by hand, and with or without a photo table."""
    rng = np.random.default_rng(seed)
    rows4 = np.array([[0, 20, 30, int(rng.integers(0, 8))]] + [[int(rng.integers(0, 2)), int(rng.integers(0, 87)), int(rng.integers(0, 108)), int(rng.integers(0, 8))]
                                                              for _ in range(B - 1)], np.int32)
    if affine:
        b = pool.affine_batch(scenes.affine_rows(rows4, 64, rng.uniform(-180, 180, B), np.exp(rng.uniform(np.log(0.7), np.log(1.4), B)),
                                                 rng.integers(-5 * 65536, 5 * 65536 + 1, (B, 2))))
    else:
        b = pool.batch(rows4)
    table = scenes.CopyPaste(CLASSES, per_window=(2, 4), over_void=True).draw(rng, pool.bank, B, 64, C)
    biggest = int(np.argmax(np.where(np.maximum(pool.bank[:, 6] - pool.bank[:, 4], pool.bank[:, 7] - pool.bank[:, 5]) < 40, pool.bank[:, 3], 0)))
    table = np.concatenate([scenes.paste_rows(pool.bank, 0, biggest, 0, 16, 16, over_void=True), table])
    b = b.with_paste(table)
    return b.with_photo(scenes.PhotoJitter(noise_sigma=(1.0, 3.0)).draw(rng, B, 3)) if photo else b


def void_engine():
    from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig
    eng = Engine(ModelConfig(input_shape=SHAPE, num_classes=C, multitasking=True, depth=6), dtype="f32", seed=7, split_k=False)
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in HEADS}, weight={h: 1.0 for h in HEADS}, ignore_void=1))
    return eng


class Recorder:
    """The names of the C ABI calls issued while it is active."""

    def __init__(self, monkeypatch):
        self.names = []
        lib = L.lib()
        inner = lib.call

        def call(name, *args):
            self.names.append(name)
            return inner(name, *args)
        monkeypatch.setattr(lib, "call", call)                                   # on the instance, as the other scene tests log it

    def take(self):
        out, self.names = self.names, []
        return out


@pytest.mark.parametrize("ignore_void", [False, True])
@pytest.mark.parametrize("photo", [False, True])
@pytest.mark.parametrize("affine", [False, True])
def test_engine_buffers_hold_the_compact_paths_bytes(pool, monkeypatch, affine, photo, ignore_void):
    """A scene batch with a paste table through _upload_scene leaves batch.host()'s bytes in g.compact_buffers(); g.x_in, every
    head's y and the void mask are what _upload_compact makes from those host bytes.  The calls: those of the batch without the
    table, and one rua_window_paste behind the cut."""
    eng = void_engine() if ignore_void else new_engine(True)
    batch = paste_batch(pool, 1, affine, photo)
    img, cls = batch.host()
    raw_img, raw_cls = batch.with_paste(None).host()
    assert not np.array_equal(img, raw_img) and not np.array_equal(cls, raw_cls)
    assert ((raw_cls >= C) & (cls < C)).any(), "no object was pasted over void"
    rec = Recorder(monkeypatch)
    for training in (True, False):
        g = eng.graph(2, training)
        outs = lambda: [g.x_in.t] + [h["y"].t for h in g.heads] + ([g.void_u8] if g.void_u8 is not None else [])
        assert (g.void_u8 is not None) == ignore_void
        eng._upload_compact(g, torch.from_numpy(img).pin_memory(), torch.from_numpy(cls).pin_memory(), 1)
        torch.cuda.synchronize()
        want = [t.clone() for t in outs()]
        if ignore_void:
            assert want[-1].any() and not want[-1].all()
        for t in outs():
            t.fill_(float("nan")) if t.is_floating_point() else t.fill_(0x77)
        for t in g.compact_buffers()[:2]:
            t.fill_(0xEE)
        rec.take()
        eng._upload_scene(g, batch, 1)
        with_table = rec.take()
        torch.cuda.synchronize()
        bi, bc = g.compact_buffers()[:2]
        assert np.array_equal(bc.cpu().numpy().reshape(cls.shape), cls) and np.array_equal(bi.cpu().numpy().reshape(img.shape), img)
        for w, v in zip(want, outs()):
            assert torch.equal(w.view(torch.uint8), v.view(torch.uint8)), (training,)
        eng._upload_scene(g, batch.with_paste(None), 1)
        without = rec.take()
        torch.cuda.synchronize()
        cut = "rua_scene_windows_affine" if affine else "rua_scene_windows"
        assert without == [cut] + (["rua_window_photometric"] if photo else []) + ["rua_multitask_targets"] + (["rua_void_mask"] if ignore_void else [])
        assert with_table == without[:1] + ["rua_window_paste"] + without[1:]
        assert np.array_equal(g.compact_buffers()[1].cpu().numpy().reshape(cls.shape), raw_cls)


def test_paste_is_refused_where_it_has_no_meaning(pool):
    eng = new_engine(False)
    batch = paste_batch(pool, 2, False, False)
    x, y = np.zeros((2, 64, 64, 3), np.float32), np.zeros((2, 64, 64, C), np.float32)
    u8 = np.zeros((2, 64, 64, 3), np.uint8)
    for step in (eng.train_step, eng.test_step, eng.forward_backward):
        with pytest.raises(ValueError, match="scene batches only"):
            step(x, y, paste=batch.paste)
        with pytest.raises(ValueError, match="scene batches only"):
            step(u8, np.zeros((2, 64, 64), np.uint8), norm_type=1, paste=batch.paste)
        with pytest.raises(ValueError, match="carries its own"):
            step(batch, None, norm_type=1, paste=batch.paste)
    m = new_training_model(False)
    with pytest.raises(ValueError, match="scene batches only"):
        m.train_on_batch(u8, np.zeros((2, 64, 64), np.uint8), norm_type=1, paste=batch.paste)
    with pytest.raises(ValueError, match="carries its own"):
        m.test_on_batch(batch, norm_type=1, paste=batch.paste)
    with pytest.raises(ValueError, match="cut without labels"):
        m.predict(batch, norm_type=1)
    other = scenes.ScenePool(pool.images, pool.class_maps, patch=64)
    other.object_bank(C + 1, CLASSES)
    with pytest.raises(ValueError, match="built for 5 classes, the model has 4"):
        eng.train_step(other.batch(batch.rows).with_paste(batch.paste[:0]), None, norm_type=1)


# ---- 3. model ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def one_block_stem():
    """The stem's weight gradient as one block: the step is then a function of its inputs (tests/test_scene_photo_gpu.py says why)."""
    lib = L.lib()
    before = lib.get_tuning("stem_blocks")
    lib.set_tuning(stem_blocks=1)
    yield
    lib.set_tuning(stem_blocks=before)


def run_steps(m, pool, how):
    """Two training steps on the same pasted windows: from scene batches that carry their tables, or from the compact batches their
    host() gives."""
    out = []
    for seed, affine, photo in ((21, False, True), (22, True, False)):
        b = paste_batch(pool, seed, affine, photo)
        out.append(m.train_on_batch(b, norm_type=1) if how == "scene" else m.train_on_batch(*b.host(), norm_type=1))
    return np.asarray(out, np.float64), state(m)


@pytest.mark.parametrize("use_graph", [True, False])
def test_model_paste_batches_train_like_compact_batches(pool, one_block_stem, monkeypatch, use_graph):
    """Two steps over the scene route and over the compact route on the same bytes: the same metrics, weights and BatchNorm state,
    bit for bit.  A step without a table issues no paste call; one with a table issues one more call than that, the paste."""
    want_metrics, want_state = run_steps(new_training_model(use_graph), pool, "host")
    assert np.isfinite(want_metrics).all()
    m = new_training_model(use_graph)
    metrics, st = run_steps(m, pool, "scene")
    print("metrics deviate by", np.abs(metrics - want_metrics).max(), "state by", np.abs(st - want_state).max())
    assert np.array_equal(metrics, want_metrics) and np.array_equal(st, want_state)
    rec = Recorder(monkeypatch)
    b = paste_batch(pool, 23, False, False)
    m.train_on_batch(b.with_paste(None), norm_type=1)
    without = rec.take()
    m.train_on_batch(b, norm_type=1)
    with_table = rec.take()
    m.train_on_batch(b.with_paste(None), norm_type=1)
    assert rec.take() == without, "a step without a table does not repeat its calls"
    cut = without.index("rua_scene_windows")
    assert "rua_window_paste" not in without
    assert with_table == without[:cut + 1] + ["rua_window_paste"] + without[cut + 1:]


# ---- 4. the object bank on the GPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"min_area": 5, "max_area": 300, "max_extent": 40}, {"connectivity": 8, "min_area": 2}])
def test_pool_object_bank_is_the_host_definition(kw):
    sc = [blob_scene(100), blob_scene(101, 97, 130)]
    p = scenes.ScenePool([s[0] for s in sc], [s[1] for s in sc], patch=64)
    bank = p.object_bank(C, CLASSES, **kw)
    want_inst, want_bank = scenes.host_object_bank([s[1] for s in sc], C, CLASSES, **dict({"max_extent": 64}, **kw))
    assert len(want_bank) > 20 and set(want_bank[:, 0].tolist()) == {0, 1} and set(want_bank[:, 2].tolist()) == set(CLASSES)
    assert bank.dtype == np.int32 and np.array_equal(bank, want_bank) and p.bank is bank and p.bank_classes == C
    assert len(p.inst_dev) == 2 and [t.data_ptr() for t in p.inst_dev] == [int(v) for v in p.inst_ptrs]
    for s in range(2):
        assert p.inst_dev[s].dtype == torch.int32 and np.array_equal(p.inst_dev[s].cpu().numpy(), want_inst[s])
        assert np.array_equal(p.inst_maps[s], want_inst[s])


# ---- 5. CLI -----------------------------------------------------------------------------------------------------------------------
def run_cli(results, dataset, extra):
    cmd = [sys.executable, os.path.join(ROOT, "train_ISPRS.py"), "--resunet_a", "yes", "--multitasking", "yes", "--loss", "tanimoto", "-rp", results,
           "-dp", dataset, "-bs", "8", "-ps", "64", "--num_classes", str(C), "--epochs", "1", "--dtype", "f32", "--norm_type", "1", "--seed", "5",
           "--stride", "32", "--data_aug", "no"] + extra
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def test_cli_paste_aug_trains_and_flag_errors_exit_before_loading(tmp_path):
    """A seeded 160 x 192 scene, -ps 64, stride 32 without the five copies: 20 windows, 16 of them trained on in two steps of one
    epoch with --paste_aug yes; the bank line is printed and the losses are finite.  A flag error ends the run before the dataset
    (a directory that does not exist) is looked at."""
    img, cls = blob_scene(200, 160, 192)
    root = str(tmp_path / "scenes")
    scenes.save_scene_dir(root, ["tile"], [img], [cls])
    r = run_cli(str(tmp_path / "a"), root, ["--scene_dataset", "yes", "--paste_aug", "yes", "--paste_classes", "1", "3", "--paste_per_window", "1", "3",
                                            "--paste_onto", "1:0,2", "--paste_min_area", "4", "--paste_max_area", "2000"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    _, want = scenes.host_object_bank([cls], C, [1, 3], min_area=4, max_area=2000, max_extent=64)
    line = [l for l in r.stdout.splitlines() if l.startswith("Object bank:")]
    assert len(line) == 1 and f"Object bank: {len(want)} objects of 1 training scenes (class 1: {int((want[:, 2] == 1).sum())}, class 3: {int((want[:, 2] == 3).sum())})" in line[0]
    tr = read_scalars(os.path.join(str(tmp_path / "a"), "logs", "train", "scalars.jsonl"))
    va = read_scalars(os.path.join(str(tmp_path / "a"), "logs", "val", "scalars.jsonl"))
    losses = [s for s in tr if s["tag"].endswith("/Loss")]
    assert losses and va and all(np.isfinite(s["value"]) for s in tr + va if s["tag"] != "Segmentation/MCC")
    bad = run_cli(str(tmp_path / "b"), str(tmp_path / "no_such_directory"), ["--paste_aug", "yes", "--paste_classes", "1"])
    assert bad.returncode != 0 and "--paste_aug yes pastes objects of resident scenes: it needs --scene_dataset yes" in bad.stderr, bad.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "b"))
    import train_ISPRS as cli
    on = ["--scene_dataset", "yes", "--num_classes", str(C), "--paste_aug", "yes"]
    for extra, message in (([], "--paste_aug yes needs --paste_classes"), (["--paste_classes", "4"], "--paste_classes 4 outside 0..3"),
                           (["--paste_classes", "1", "--paste_onto", "3:0"], "class 3 is not one of --paste_classes"),
                           (["--paste_classes", "1", "--paste_onto", "1-0"], "SRC:DST"), (["--paste_classes", "1", "--paste_onto", "1:7"], "destination class outside 0..3"),
                           (["--paste_classes", "1", "--paste_per_window", "3", "1"], "per_window range"),
                           (["--paste_classes", "1", "--paste_min_area", "9", "--paste_max_area", "3"], "1 <= min <= max")):
        with pytest.raises(SystemExit, match=message):
            cli.check_paste_flags(cli.build_parser().parse_args(on + extra))
    cp = cli.check_paste_flags(cli.build_parser().parse_args(on + ["--paste_classes", "3", "1", "--paste_onto", "1:0,2", "3:0", "--paste_over_void", "yes"]))
    assert cp.classes == (1, 3) and cp.onto == {1: [0, 2], 3: [0]} and cp.over_void and cp.per_window == (0, 3)
    assert cli.check_paste_flags(cli.build_parser().parse_args([])) is None
