"""The chooser between the two forms of the fused BatchNorm launches (csrc/elementwise.hip, bn_route) through its route queries rua_bn_fwd_route /
rua_bn_bwd_route and rua_bn_part_range: no GPU, nothing is launched.  A route is 0 (pixel-major) or S | P << 8 (channel-sliced: blocks own S 16-byte pieces per
pixel of one of P contiguous pixel parts)."""
import contextlib
import ctypes as C

import pytest

from resunet_a_mltsk_keras_amd import _lib as L

F32, BF16 = L.RUA_F32, L.RUA_BF16
CHANNELS = [8, 32, 64, 72, 192, 256, 1024, 2048]
PIXELS = list(range(1, 71)) + [255, 256, 257, 258, 512, 8192, 65536]
OUT_R = [0, 1, 4, 32]                                        # replicas of the launch's statistics outputs (0: none)


def vec(dt):
    return 8 if dt == BF16 else 4


@contextlib.contextmanager
def tuning(**kv):
    lib = L.lib()
    before = {k: lib.get_tuning(k) for k in kv}
    try:
        lib.set_tuning(**kv)
        yield
    finally:
        lib.set_tuning(**before)


def fwd_route(M, Cc, dt, nb=1, out=True, training=1, replicas=1):
    d = L.BnFwdDesc()
    d.M, d.C, d.dtype, d.nb, d.training, d.replicas, d.stats, d.count = M, Cc, dt, nb, training, replicas, 64, float(M)
    for b in range(nb):
        d.br[b].out = 64 if out else None                    # (addresses are never followed by a route query)
    return L.lib().raw("rua_bn_fwd_route")(C.byref(d))


def bwd_route(M, Cc, dt, nb=1, skip_r=0, dx_r=0, replicas=1):
    e = L.BnBwdDesc()
    e.M, e.C, e.dtype, e.nb, e.count = M, Cc, dt, nb, float(M)
    for b in range(nb):
        e.br[b].replicas = replicas
    if skip_r:
        e.skip_stats, e.skip_replicas = 64, skip_r
    if dx_r:
        e.dx_stats, e.dx_replicas = 64, dx_r
    return L.lib().raw("rua_bn_bwd_route")(C.byref(e))


def parts_of(M, P):
    lib, a, b = L.lib(), C.c_int64(), C.c_int64()
    out = []
    for part in range(P):
        lib.call("rua_bn_part_range", M, P, part, C.byref(a), C.byref(b))
        out.append((a.value, b.value))
    return out


def check_route(r, M, Cc, dt, out_r):
    """What every sliced route has to satisfy; returns (S, P)."""
    S, P = r & 255, r >> 8
    assert S in (4, 8) and Cc % (S * vec(dt)) == 0
    slices = Cc // (S * vec(dt))
    assert slices >= 1 and slices * S * vec(dt) == Cc
    assert 1 <= P <= M
    if out_r:
        assert P <= out_r, "one add per address of a statistics output"
    pr = parts_of(M, P)
    assert pr[0][0] == 0 and pr[-1][1] == M
    assert all(a < b for a, b in pr), "an empty part"
    assert all(pr[i][1] == pr[i + 1][0] for i in range(P - 1)), "a pixel twice or missing"
    return S, P


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", CHANNELS)
def test_routes_tile_the_tensor(Cc, dt):
    sliced = 0
    for M in PIXELS:
        for r_out in OUT_R:
            routes = [bwd_route(M, Cc, dt, nb=3, skip_r=r_out, dx_r=32 if r_out else 0, replicas=8)]
            if r_out == 0:
                routes += [fwd_route(M, Cc, dt, nb=2), fwd_route(M, Cc, dt, training=0)]
            for r in routes:
                if Cc % (4 * vec(dt)) != 0:
                    assert r == 0, "no whole slice of 4 or 8 pieces"
                elif r:
                    S, _ = check_route(r, M, Cc, dt, r_out)
                    assert S == (8 if Cc % (8 * vec(dt)) == 0 else 4), "whole 128-byte lines wherever they fit"
                    sliced += 1
    if Cc % (4 * vec(dt)) == 0:
        assert sliced > 0


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_small_maps_are_sliced_and_large_ones_are_not(dt):
    """cfg3's deep shapes take the sliced form; the launches of levels 1 - 3 (2^16 x 32 ... 2^15 x 128 in bf16 terms) stay pixel-major, and so does a launch whose statistics
    output has too few replicas for its pixels (its blocks would sweep more than eight steps each)."""
    k = 8 // vec(dt)                                         # the same bytes in either type
    for M, Cc in ((512, 1024), (2048, 512), (8192, 256), (8, 256), (32, 256), (128, 256)):
        assert fwd_route(M, Cc // k, dt) != 0 and bwd_route(M, Cc // k, dt, nb=1) != 0
        assert bwd_route(M, Cc // k, dt, nb=3, skip_r=32, dx_r=32) != 0
    for M, Cc in ((524288, 32), (131072, 64), (32768, 128), (65536, 256)):
        assert fwd_route(M, Cc // k, dt) == 0 and bwd_route(M, Cc // k, dt, nb=1) == 0
    assert bwd_route(8192, 256 // k, dt, skip_r=1) == 0 and bwd_route(256, 256 // k, dt, skip_r=1) != 0


def test_what_is_not_eligible_reports_zero():
    assert fwd_route(64, 64, BF16, out=False) == 0, "coefficient-only launches stay one block"
    assert fwd_route(64, 64, 7) == 0 and bwd_route(64, 64, -1) == 0
    assert fwd_route(64, 64, BF16, nb=0) == 0 and bwd_route(64, 64, BF16, nb=0) == 0
    assert fwd_route(0, 64, BF16) == 0 and bwd_route(0, 64, BF16) == 0
    assert L.lib().raw("rua_bn_fwd_route")(None) == 0 and L.lib().raw("rua_bn_bwd_route")(None) == 0
    a, b = C.c_int64(), C.c_int64()
    part_range = L.lib().raw("rua_bn_part_range")
    assert part_range(5, 6, 0, C.byref(a), C.byref(b)) != 0 and part_range(5, 5, 5, C.byref(a), C.byref(b)) != 0 and part_range(5, 0, 0, C.byref(a), C.byref(b)) != 0


def test_the_key_switches_every_route_off():
    with tuning(bn_sliced=0):
        for dt in (F32, BF16):
            for Cc in CHANNELS:
                for M in PIXELS:
                    assert fwd_route(M, Cc, dt) == 0 and bwd_route(M, Cc, dt) == 0 and bwd_route(M, Cc, dt, nb=4, skip_r=32) == 0


def test_forced_parts_tile_unevenly():
    """bn_sliced_parts (experiments and tests): any P up to M; 1000 pixels in 7 parts are 142 or 143 each."""
    with tuning(bn_sliced_parts=7):
        S, P = check_route(bwd_route(1000, 64, BF16, skip_r=4), 1000, 64, BF16, 0)
        assert P == 7 and sorted({b - a for a, b in parts_of(1000, 7)}) == [142, 143]
        assert check_route(fwd_route(3, 64, BF16), 3, 64, BF16, 0)[1] == 3
