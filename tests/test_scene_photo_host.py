"""CPU tests of the photometric jitter: scenes.host_photometric against hand values, the noise goldens and a scalar restatement in
Python integers; the behaviour of its parts; rua_window_photometric's refusals without a launch and check_photo_table's same words;
SceneBatch / AffineSceneBatch carrying a photo table; SceneLoader(photo=)."""
import numpy as np
import pytest

from resunet_a_mltsk_keras_amd import _lib as L
from resunet_a_mltsk_keras_amd import scenes

Q = 65536
IDENT = np.array([Q, 0, 0, 0, Q, 0, 0, 0, Q, 0, 0, 0, 0, 0, 0, 0], np.int32)
# (seed, idx) -> (x after mixing, z, (8868 * z + 32768) >> 16): a CPU run of a pure-Python restatement of the definition
NOISE_GOLDEN = [(0, 0, 0x01FCE552, 54, 7), (1, 0, 0x9F505634, -133, -18), (1, 1, 0x43C5316A, -91, -12),
                (-5, 1000, 0xE67DC403, 44, 6), (123456789, 786431, 0x54EE4D15, -90, -12)]


def row(**kw):
    r = IDENT.astype(np.int64)
    for k, v in kw.items():
        r[int(k[1:])] = v
    return r


def clamp(v):
    return min(max(v, 0), 255)


def mix(seed, idx):
    x = (seed + (idx + 1) * 0x9E3779B9) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x, (x & 255) + ((x >> 8) & 255) + ((x >> 16) & 255) + (x >> 24) - 510


def scalar_photometric(img, table):
    """The definition byte by byte in Python integers (their >> is arithmetic, nothing overflows)."""
    N, PH, PW, Cin = img.shape
    out = np.empty_like(img)
    for n in range(N):
        R = [int(v) for v in table[n]]
        for i in range(PH):
            for j in range(PW):
                p = [int(v) for v in img[n, i, j]]
                for c in range(Cin):
                    if Cin == 3:
                        u = clamp((R[3 * c] * p[0] + R[3 * c + 1] * p[1] + R[3 * c + 2] * p[2] + R[9 + c] + 32768) >> 16)
                    else:
                        u = clamp((R[0] * p[c] + R[9] + 32768) >> 16)
                    v = clamp(u + ((R[12] * u * (255 - u) + (1 << 23)) >> 24))
                    if R[13]:
                        _, z = mix(R[14] & 0xFFFFFFFF, (i * PW + j) * Cin + c)
                        v = clamp(v + ((R[13] * z + 32768) >> 16))
                    out[n, i, j, c] = v
    return out


def limit_rows(rng, n, scalar=False):
    """n rows random within the limits; the first ones sit AT each limit, then an identity row, a row with A = 0 and one with t = 0."""
    t = np.zeros((n, 16), np.int64)
    t[:, :9] = rng.integers(-(1 << 20), (1 << 20) + 1, (n, 9))
    t[:, 9:12] = rng.integers(-(1 << 29), (1 << 29) + 1, (n, 3))
    t[:, 12] = rng.integers(-Q, Q + 1, n)
    t[:, 13] = rng.integers(0, Q + 1, n)
    t[:, 14] = rng.integers(-(1 << 31), 1 << 31, n)
    # moderate rows too: a matrix at the limits saturates nearly every byte
    for k in range(0, n, 2):
        t[k, :9] = (np.eye(3) * Q).ravel().astype(np.int64) + rng.integers(-20000, 20001, 9)
        t[k, 9:12] = rng.integers(-40 * Q, 40 * Q + 1, 3)
        t[k, 13] = rng.integers(0, 4000)
    special = [row(r0=1 << 20, r4=-(1 << 20), r8=1 << 20, r1=1 << 20, r2=1 << 20, r9=1 << 29, r10=-(1 << 29), r11=1 << 29, r12=Q, r13=Q, r14=-1),
               row(r0=-(1 << 20), r3=-(1 << 20), r6=(1 << 20), r9=-(1 << 29), r12=-Q, r13=Q, r14=(1 << 31) - 1),
               row(), row(r0=70000, r9=-5 * Q, r12=30000, r13=0, r14=77), row(r4=50000, r10=9 * Q, r12=0, r13=3000, r14=-(1 << 31))]
    for k, r in enumerate(special[:n]):
        t[k] = r
    if scalar:
        t[:, 1:4] = t[:, 5:8] = 0
        t[:, 4] = t[:, 8] = t[:, 0]
        t[:, 10] = t[:, 11] = t[:, 9]
        if n > 2:
            t[2] = IDENT
    return t.astype(np.int32)


# ---- 1. defaults and hand values ------------------------------------------------------------------------------------------------
def test_defaults_are_the_identity_row():
    t = scenes.photo_rows(3)
    assert t.dtype == np.int32 and t.shape == (3, 16) and (t == IDENT).all()
    img = np.random.default_rng(0).integers(0, 256, (3, 6, 5, 3)).astype(np.uint8)
    assert np.array_equal(scenes.host_photometric(img, t), img)
    one = np.random.default_rng(1).integers(0, 256, (3, 6, 5, 1)).astype(np.uint8)
    assert np.array_equal(scenes.host_photometric(one, t), one)


def test_hand_values_gain_and_tone():
    px = lambda v: np.full((1, 1, 1, 3), v, np.uint8)
    gain2 = scenes.photo_rows(1, contrast=2.0, brightness=0.5)       # b = 127.5 - 127.5 = 0: a pure gain of 2
    assert gain2[0, 0] == 2 * Q and gain2[0, 9] == 0
    assert scenes.host_photometric(px(100), gain2).ravel().tolist() == [200] * 3
    assert scenes.host_photometric(px(200), gain2).ravel().tolist() == [255] * 3
    assert scenes.host_photometric(px(128), scenes.photo_rows(1, tone=1.0)).ravel().tolist() == [192] * 3
    assert scenes.host_photometric(px(128), scenes.photo_rows(1, tone=-1.0)).ravel().tolist() == [65] * 3
    for v in (0, 255):
        for tone in (1.0, -1.0):
            assert scenes.host_photometric(px(v), scenes.photo_rows(1, tone=tone)).ravel().tolist() == [v] * 3


def test_noise_goldens():
    A = 8868
    assert A == int(np.rint(Q * 20.0 / scenes.SIGMA_Z)) and abs(scenes.SIGMA_Z - 147.80) < 0.01
    for seed, idx, x, z, delta in NOISE_GOLDEN:
        assert mix(seed & 0xFFFFFFFF, idx) == (x, z)
        assert (A * z + 32768) >> 16 == delta
        # through host_photometric: byte idx of a 512 x 512 x 3 window holding 128 everywhere
        img = np.full((1, 512, 512, 3), 128, np.uint8)
        out = scenes.host_photometric(img, row(r13=A, r14=seed)[None])
        assert int(out.ravel()[idx]) == 128 + delta, (seed, idx)
    # z is the sum of four bytes minus 510: its standard deviation over many draws is sqrt((256^2 - 1) / 3) within 1 %
    zs = np.array([mix(12345, i)[1] for i in range(20000)])
    assert zs.min() >= -510 and zs.max() <= 510 and abs(zs.mean()) < 4 and abs(zs.std() / scenes.SIGMA_Z - 1) < 0.02


@pytest.mark.parametrize("Cin", [3, 1, 4])
def test_scalar_restatement_agrees_at_the_limits(Cin):
    rng = np.random.default_rng(5 + Cin)
    table = limit_rows(rng, 8, scalar=Cin != 3)
    img = rng.integers(0, 256, (8, 5, 7, Cin)).astype(np.uint8)
    img[0, 0, 0], img[1, 0, 0] = 255, 0
    got = scenes.host_photometric(img, table)
    assert got.dtype == np.uint8 and np.array_equal(got, scalar_photometric(img, table))


# ---- 2. behaviour of the parts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tone", [1.0, -1.0])
def test_tone_curve_is_monotone(tone):
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1)
    out = scenes.host_photometric(ramp, scenes.check_photo_table(scenes.photo_rows(1, tone=tone), 1)).ravel().astype(int)
    assert out[0] == 0 and out[255] == 255 and (np.diff(out) >= 0).all()
    assert (out >= np.arange(256)).all() if tone > 0 else (out <= np.arange(256)).all()


def test_grey_stays_grey_under_saturation_and_hue():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, None, :, None], 3, axis=3)
    out = scenes.host_photometric(grey, scenes.photo_rows(1, saturation=1.7, hue_deg=77.0)).astype(int)
    assert np.abs(out - grey.astype(int)).max() <= 1
    colour = np.array([[[[200, 30, 90]]]], np.uint8)             # while a colour does move
    assert np.abs(scenes.host_photometric(colour, scenes.photo_rows(1, hue_deg=77.0)).astype(int) - colour).max() > 20


def test_noise_depends_on_seed_and_window_position_only():
    rng = np.random.default_rng(9)
    w = rng.integers(40, 216, (1, 9, 11, 3)).astype(np.uint8)
    other = rng.integers(0, 256, (1, 9, 11, 3)).astype(np.uint8)
    noisy = scenes.photo_rows(1, noise_sigma=6.0, seeds=4242)[0]
    first = scenes.host_photometric(np.concatenate([w, other, other]), np.stack([noisy, IDENT, IDENT]))[0]
    last = scenes.host_photometric(np.concatenate([other, other, w]), np.stack([IDENT, IDENT, noisy]))[2]
    assert np.array_equal(first, last) and not np.array_equal(first, w[0])
    reseeded = scenes.host_photometric(w, scenes.photo_rows(1, noise_sigma=6.0, seeds=4243))[0]
    assert not np.array_equal(first, reseeded)
    d = first.astype(int) - w[0]
    assert abs(d.std() - 6.0) < 1.0 and abs(d.mean()) < 1.0


# ---- 3. refusals without a launch -----------------------------------------------------------------------------------------------
def test_photometric_argument_validation_without_launch():
    """Every case breaks exactly one precondition of a valid call, so none of them reaches a launch; check_photo_table refuses the
    same tables in the same words."""
    lib = L.lib()
    fn = lib.raw("rua_window_photometric")
    A = 1 << 24                                               # fake, suitably aligned addresses: never dereferenced on the host
    good = np.stack([row(r0=1 << 20, r9=-(1 << 29), r12=Q, r13=Q, r14=-7), row(r4=-(1 << 20), r11=1 << 29, r12=-Q)]).astype(np.int32)

    def call(table, img_in=A, img_out=A, N=None, PH=8, PW=8, Cin=3, photo=True):
        t = np.ascontiguousarray(table, dtype=np.int32)
        return fn(img_in, img_out, len(t) if N is None else N, PH, PW, Cin, t.ctypes.data if photo else None, None)

    def last():
        return lib.dll.rua_last_error().decode()

    assert np.array_equal(scenes.check_photo_table(good, 3), good)           # the limits themselves are inside
    scalar_good = np.stack([row(r0=1 << 20, r4=1 << 20, r8=1 << 20, r9=1 << 29, r10=1 << 29, r11=1 << 29, r12=Q, r13=Q)]).astype(np.int32)
    for ch in (1, 4, 16):
        assert np.array_equal(scenes.check_photo_table(scalar_good, ch), scalar_good)

    general = [(dict(img_in=None), "required"), (dict(img_out=None), "required"), (dict(photo=False), "required"),
               (dict(img_out=A + 2, img_in=A + 2), "4-byte"), (dict(img_out=A + 2 + (1 << 20)), "4-byte"),
               (dict(img_out=A + 4), "overlap in part"), (dict(img_in=A + 8 * 8 * 3 * 2 - 4), "overlap in part"),
               (dict(N=0), "N 0"), (dict(Cin=0), "Cin 0"), (dict(Cin=17), "Cin 17"), (dict(PH=513), "512"), (dict(PW=0), "512")]
    for change, msg in general:
        assert call(good, **change) == -1, change
        assert msg in last() and last().startswith("rua_window_photometric: "), (change, last())
    big = np.tile(scalar_good, (512, 1))
    assert call(big, PH=512, PW=512, Cin=16) == -1 and "2^31" in last()
    with pytest.raises(ValueError, match=r"N 0 \(>= 1\)"):
        scenes.check_photo_table(np.zeros((0, 16), np.int32), 3)
    for ch in (0, 17):
        assert call(good, Cin=ch) == -1
        with pytest.raises(ValueError) as exc:
            scenes.check_photo_table(good, ch)
        assert str(exc.value) == last()
    with pytest.raises(ValueError, match=r"integer \[N\]\[16\]"):
        scenes.check_photo_table(np.zeros((2, 15), np.int32), 3)

    # each limit of the table exceeded by one, in the second row; the reserved word; the words name the row and the word
    cases = [(q, s * ((1 << 20) + 1), "matrix entry") for q in range(9) for s in (1, -1)]
    cases += [(q, s * ((1 << 29) + 1), "offset") for q in (9, 10, 11) for s in (1, -1)]
    cases += [(12, Q + 1, "tone"), (12, -Q - 1, "tone"), (13, Q + 1, "noise amplitude"), (13, -1, "noise amplitude"), (15, 1, "reserved"), (15, -3, "reserved")]
    for q, v, what in cases:
        bad = good.copy()
        bad[1, q] = v
        assert call(bad) == -1, (q, v)
        err = last()
        assert f"row 1: word {q}: " in err and what in err and str(v) in err, err
        with pytest.raises(ValueError) as exc:
            scenes.check_photo_table(bad, 3)
        assert str(exc.value) == err

    # Cin != 3 takes scalar rows only
    for q, v in [(1, 5), (3, -1), (7, 1), (4, (1 << 20) - 1), (8, 0), (10, 1 << 28), (11, 0)]:
        bad = np.concatenate([scalar_good, scalar_good])
        bad[1, q] = v
        assert call(bad, Cin=4) == -1, (q, v)
        err = last()
        assert f"row 1: word {q}: {v}, but Cin 4 != 3 takes scalar rows" in err, err
        with pytest.raises(ValueError) as exc:
            scenes.check_photo_table(bad, 4)
        assert str(exc.value) == err
        assert np.array_equal(scenes.check_photo_table(bad, 3), bad)         # a full row is fine at three channels
    with pytest.raises(ValueError, match="row 0: word 4: 65536, but Cin 4"):
        scenes.host_photometric(np.zeros((2, 4, 4, 4), np.uint8), good)


# ---- 4. SceneBatch plumbing -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_pool():
    rng = np.random.default_rng(3)
    shapes = [(70, 81), (64, 90)]
    return scenes.ScenePool([rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in shapes],
                            [rng.integers(0, 5, s).astype(np.uint8) for s in shapes], patch=32, device="cpu")


def batches(pool, n=6):
    rng = np.random.default_rng(11)
    rows4 = np.array([[k % 2, int(rng.integers(0, 30)), int(rng.integers(0, 40)), k % 8] for k in range(n)], np.int32)
    t7 = scenes.affine_rows(rows4, 32, rng.uniform(-180, 180, n), np.exp(rng.uniform(-0.5, 0.5, n)), rng.integers(-5 * Q, 5 * Q, (n, 2)))
    return pool.batch(rows4), pool.affine_batch(t7)


@pytest.mark.parametrize("affine", [False, True])
def test_batches_carry_their_photo_table(cpu_pool, affine):
    plain = batches(cpu_pool)[int(affine)]
    assert plain.photo is None
    table = scenes.PhotoJitter().draw(np.random.default_rng(2), len(plain), 3)
    b = plain.with_photo(table)
    assert type(b) is type(plain) and b.photo.dtype == np.int32 and np.array_equal(b.photo, table) and np.array_equal(b.rows, plain.rows)
    assert plain.photo is None and b.shape == plain.shape
    img0, cls0 = plain.host()
    img, cls = b.host()
    assert np.array_equal(img, scenes.host_photometric(img0, table)) and not np.array_equal(img, img0)
    assert np.array_equal(cls, cls0)
    part = b[1:5]
    assert type(part) is type(plain) and np.array_equal(part.rows, plain.rows[1:5]) and np.array_equal(part.photo, table[1:5])
    assert np.array_equal(part.host()[0], img[1:5])
    for r in range(3):
        sh = b.shard(r, 3)
        assert np.array_equal(sh.rows, plain.rows[2 * r:2 * r + 2]) and np.array_equal(sh.photo, table[2 * r:2 * r + 2])
        assert np.array_equal(sh.host()[0], img[2 * r:2 * r + 2])
    assert plain[1:3].photo is None and b.with_photo(None).photo is None
    with pytest.raises(ValueError, match="photo rows for a batch"):
        plain.with_photo(table[:-1])
    bad = table.copy()
    bad[2, 15] = 1
    with pytest.raises(ValueError, match="row 2: word 15"):
        plain.with_photo(bad)


# ---- 5. SceneLoader(photo=) -----------------------------------------------------------------------------------------------------
def loader_tables(pool, world=1, rank=0, passes=1, **kw):
    table = scenes.window_table(pool.shapes, 32, 16, True)
    ld = scenes.SceneLoader(pool, table, 4, rank=rank, world=world, order=np.arange(16), **kw)
    out = []
    for _ in range(passes):
        out.append([b for b, y in ld])
        assert len(out[-1]) == 4
    return out


def test_loader_draws_photo_tables(cpu_pool):
    pj = scenes.PhotoJitter()
    (p0, p1), = [loader_tables(cpu_pool, passes=2, photo=pj, seed=7)]
    again = loader_tables(cpu_pool, passes=2, photo=pj, seed=7)
    for e, batches_ in enumerate((p0, p1)):
        for k, b in enumerate(batches_):
            assert type(b) is scenes.SceneBatch and b.photo.shape == (4, 16) and b.photo.dtype == np.int32
            assert np.array_equal(b.photo, again[e][k].photo) and np.array_equal(b.rows, again[e][k].rows)
            assert np.array_equal(b.photo, pj.draw(np.random.default_rng([7, e, k, 1]), 4, 3))
    assert all(not np.array_equal(a.photo, b.photo) for a, b in zip(p0, p1))          # pass 1 differs from pass 0
    assert all(np.array_equal(a.rows, b.rows) for a, b in zip(p0, p1))
    other = loader_tables(cpu_pool, photo=pj, seed=8)[0]
    assert all(not np.array_equal(a.photo, b.photo) for a, b in zip(p0, other))
    # two ranks of a world of 2, concatenated, are the world of 1
    r0, r1 = (loader_tables(cpu_pool, world=2, rank=r, photo=pj, seed=7)[0] for r in (0, 1))
    for k, b in enumerate(p0):
        assert np.array_equal(np.concatenate([r0[k].photo, r1[k].photo]), b.photo)
        assert np.array_equal(np.concatenate([r0[k].rows, r1[k].rows]), b.rows)
        assert np.array_equal(np.concatenate([r0[k].host()[0], r1[k].host()[0]]), b.host()[0])
    # without photo: today's batches
    for b, today in zip(loader_tables(cpu_pool, seed=7)[0], loader_tables(cpu_pool)[0]):
        assert b.photo is None and np.array_equal(b.rows, today.rows)


def test_loader_photo_leaves_the_geometric_draws_alone(cpu_pool):
    jit = scenes.Jitter(30.0, (0.9, 1.1), 4.0)
    both = loader_tables(cpu_pool, passes=2, jitter=jit, photo=scenes.PhotoJitter(), seed=3)
    geo = loader_tables(cpu_pool, passes=2, jitter=jit, seed=3)
    for e in range(2):
        for a, b in zip(both[e], geo[e]):
            assert type(a) is scenes.AffineSceneBatch and np.array_equal(a.rows, b.rows) and b.photo is None and a.photo.shape == (4, 16)
    assert not np.array_equal(both[0][0].photo, both[1][0].photo)


def test_photo_jitter_draw():
    pj = scenes.PhotoJitter()
    t3 = pj.draw(np.random.default_rng(1), 64, 3)
    t1 = pj.draw(np.random.default_rng(1), 64, 1)
    assert t3.shape == t1.shape == (64, 16) and t3.dtype == t1.dtype == np.int32
    assert np.array_equal(t3[:, 9:], t1[:, 9:])                  # the same draws; saturation and hue stay out of scalar rows
    assert (t1[:, [1, 2, 3, 5, 6, 7]] == 0).all() and (t1[:, 0] == t1[:, 4]).all() and (t1[:, 0] == t1[:, 8]).all()
    assert (t3[:, [1, 2, 3, 5, 6, 7]] != 0).any()
    assert (np.abs(t3[:, 9] - (1 - t1[:, 0] / Q) * 127.5 * Q) <= 0.1 * 255 * Q + 1).all()
    assert (t1[:, 0] >= int(0.8 * Q) - 1).all() and (t1[:, 0] <= int(1.25 * Q) + 1).all()
    assert (np.abs(t3[:, 12]) <= 0.4 * Q + 1).all() and (t3[:, 13] >= 0).all() and (t3[:, 13] <= 3.0 / scenes.SIGMA_Z * Q + 1).all()
    assert (t3[:, 14] >= 0).all() and len(set(t3[:, 14].tolist())) == 64 and (t3[:, 15] == 0).all()
    off = scenes.PhotoJitter(0, (1, 1), (1, 1), 0, 0, (0, 0)).draw(np.random.default_rng(1), 5, 3)
    assert (off[:, :14] == IDENT[:14]).all()
