"""What the tests/test_scene*_gpu.py files share: the blob scenes and small models of the engine-level tests, the window tables
and pre-filled buffers of the C ABI tests.  A plain module (no tests, no fixtures): the test files import from it by name."""
import json

import numpy as np

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

HEADS = ["seg", "bound", "dist", "color"]
SHAPE, NCLS = (64, 64, 3), 4                                 # the engine-level tests: 64 x 64 patches, four classes
GUARD = 4096                                                 # bytes behind each output that must come back untouched
FILL = 0xEE                                                  # what a scene map holds before a call


def table_of(shapes, patch, stride):
    """predict_table of every scene, concatenated: (rows, own) with the scene index in column 0."""
    parts = []
    for s, shp in enumerate(shapes):
        rows, own = scenes.predict_table(shp, patch, stride)
        rows[:, 0] = s
        parts.append((rows, own))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def conf_pattern(C):
    return (np.arange(C * C, dtype=np.int64).reshape(C, C) * 7 + 3) * (1 << 33) + 5      # non-zero in both halves of every cell


def guarded_maps(shapes, channels=1):
    """One FILL-ed uint8 device buffer per scene: H * W * channels bytes and GUARD bytes behind them."""
    import torch
    return [torch.full((H * W * channels + GUARD,), FILL, dtype=torch.uint8, device="cuda") for H, W in shapes]


def read_guarded(bufs, shapes, channels=None):
    """The maps out of guarded_maps' buffers, [H][W] (channels=None) or [H][W][channels]; the bytes behind each must still hold FILL."""
    out = []
    for t, (H, W) in zip(bufs, shapes):
        g, n = t.cpu().numpy(), H * W * (channels or 1)
        assert (g[n:] == FILL).all(), "bytes behind a scene map were written"
        out.append(g[:n].reshape((H, W) if channels is None else (H, W, channels)))
    return out


def make_scenes(rng, shapes, Cin):
    return ([rng.integers(0, 256, (H, W, Cin)).astype(np.uint8) for H, W in shapes],
            [rng.integers(0, 256, (H, W)).astype(np.uint8) for H, W in shapes])


def assert_same(got, want, table, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), "first at", tuple(bad[0]), "table row", table[bad[0][0]].tolist())


def blob_scene(seed, H=150, W=171):
    """An image with pure hues and a grey pixel, a blocky class map with speckle (as tests/test_targets_gpu.py builds its patches)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    img[::17, ::13] = [255, 0, 0]
    img[5::19, 3::11] = [7, 7, 7]
    f = rng.integers(0, NCLS, (H // 8 + 2, W // 8 + 2))
    cls = np.kron(f, np.ones((8, 8), np.int64))[:H, :W]
    cls[rng.random(cls.shape) < 0.01] = int(rng.integers(0, NCLS))
    return img, cls.astype(np.uint8)


def blob_pool(second=(150, 171)):
    """A ScenePool of blob_scene(100) and a blob_scene(101) of the shape `second`, patch 64."""
    sc = [blob_scene(100), blob_scene(101, *second)]
    return scenes.ScenePool([s[0] for s in sc], [s[1] for s in sc], patch=64)


def new_engine(multitask, use_graph=None, seed=7, shape=SHAPE, depth=6):
    """A compiled f32 Engine without split-K; use_graph None leaves the engine's own choice."""
    from resunet_a_mltsk_keras_amd.engine import Engine, LossSpec, ModelConfig
    heads = HEADS if multitask else ["seg"]
    eng = Engine(ModelConfig(input_shape=shape, num_classes=NCLS, multitasking=multitask, depth=depth), dtype="f32", seed=seed, split_k=False)
    if use_graph is not None:
        eng.use_graph = use_graph
    eng.compile(LossSpec(kind={h: L.LOSS_TANIMOTO for h in heads}, weight={h: 1.0 for h in heads}))
    return eng


def new_model(seed=3, depth=6, split_k=False):
    """A multitask f32 Model for prediction (not compiled)."""
    from resunet_a_mltsk_keras_amd.engine import ModelConfig
    from resunet_a_mltsk_keras_amd.keras_api import Model
    m = Model(ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=True, depth=depth), dtype="f32", seed=seed)
    m.engine.split_k = split_k
    return m


def new_training_model(use_graph, seed=3):
    """A multitask f32 Model compiled as train_ISPRS.py compiles it: Adam, the dual Tanimoto loss on every head."""
    from multitasking_utils import Tanimoto_dual_loss
    from resunet_a_mltsk_keras_amd.engine import ModelConfig
    from resunet_a_mltsk_keras_amd.keras_api import Adam, Model
    m = Model(ModelConfig(input_shape=SHAPE, num_classes=NCLS, multitasking=True), dtype="f32", seed=seed)
    m.engine.split_k = False
    m.engine.use_graph = use_graph
    loss = Tanimoto_dual_loss()
    m.compile(optimizer=Adam(lr=1e-3, beta_1=0.9), loss={h: loss for h in HEADS}, loss_weights={h: 1.0 for h in HEADS},
              metrics={"seg": ["accuracy"]})
    return m


def state(m):
    return np.concatenate([m.engine.P.detach().cpu().numpy().ravel(), m.engine.S.detach().cpu().numpy().ravel()])


def read_scalars(path):
    with open(path) as f:
        return [json.loads(l) for l in f]
