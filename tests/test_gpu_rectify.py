"""GPU tests of the rectifier: yv_rectify_run equals the numpy specification of tests/rectify_reference.py byte for
byte over shapes, maps, strides, pointer alignments and image counts, through the LDS-staged kernel and the direct one;
no byte outside the destination rows is written; yv_rectify_set_model gives the specification's map entry for entry; and
a run followed by yv_batch_run on the same stream without a synchronisation feeds the batch the rectified images."""
import functools

import numpy as np
import pytest

import ya_vo_amd as yv
from ya_vo_amd import io as yio
from ya_vo_amd.synth import synth_frame

import rectify_reference as rr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (9, 9, 9, 9), (33, 61, 20, 40), (120, 127, 120, 127), (120, 128, 120, 128), (64, 300, 200, 320)]
BIG = SHAPES[3:]  # a random map's box spans the source: more than 64 rows or more than 16 KiB
KINDS = ["identity", "shift", "half", "outside", "random", "rotation", "split", "kitti_raw", "full", "horizon"]
FILL = 0xA5
GUARD = 64


@functools.lru_cache(maxsize=None)
def _map(kind, shape):
    """The specification's map of a kind at a shape (read-only, shared)."""
    Hs, Ws, H, W = shape
    if kind == "identity":
        m = rr.identity_map(H, W)
    elif kind == "shift":  # half of the image comes from outside, on both axes
        m = rr.identity_map(H, W, 32 * (Ws // 2), -32 * ((Hs + 1) // 2))
    elif kind == "half":
        m = rr.identity_map(H, W, 16, 0)
    elif kind == "outside":
        m = rr.outside_map(H, W)
    elif kind == "random":
        m = rr.random_map(Hs, Ws, H, W, 11)
    elif kind == "rotation":
        m = rr.rotation_map(Hs, Ws, H, W)
    elif kind == "split":
        m = rr.split_map(Hs, Ws, H, W, 12)
    else:
        m = rr.model_map_q5(*rr.MODELS[kind](Hs, Ws, H, W), H, W)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _sources(Hs, Ws, n):
    s = np.random.default_rng(1000 * Hs + Ws).integers(0, 256, (n, Hs, Ws), dtype=np.uint8)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _expected(kind, shape, i):
    """Image i of _sources through the kind's map."""
    Hs, Ws, H, W = shape
    e = rr.remap(_sources(Hs, Ws, 37)[i], _map(kind, shape))
    e.setflags(write=False)
    return e


def _set(rect, m, kind, shape):
    if kind in rr.MODELS:
        rect.set_model(m, *rr.MODELS[kind](*shape))
    else:
        rect.set_map(m, _map(kind, shape))


def _run(rect, shape, kinds, n, ss=None, ds=None, so=0, do=0):
    """n images through the rectifier's maps (image i: map i % len(kinds), set from kinds) with rows ss / ds bytes
    apart and base pointers so / do bytes off a dword; both buffers end with the last image's last pixel, the
    destination's is followed by a guard.  Asserts the whole destination buffer: the specification's images in the rows,
    the fill everywhere else."""
    import torch
    Hs, Ws, H, W = shape
    ss, ds = ss or Ws, ds or W
    sp, dp = Hs * ss, H * ds
    src_len = so + (n - 1) * sp + (Hs - 1) * ss + Ws if n else so + 1
    dst_len = do + (n - 1) * dp + (H - 1) * ds + W if n else do + 1
    h_src = np.full(src_len, 0x5A, np.uint8)
    want = np.full(dst_len + GUARD, FILL, np.uint8)
    for i in range(n):
        s = np.lib.stride_tricks.as_strided(h_src[so + i * sp:], (Hs, Ws), (ss, 1))
        s[:] = _sources(Hs, Ws, 37)[i]
        d = np.lib.stride_tricks.as_strided(want[do + i * dp:], (H, W), (ds, 1))
        d[:] = _expected(kinds[i % len(kinds)], shape, i)
    d_src = torch.from_numpy(h_src).to("cuda:0")
    outs = []
    for force in (False, True):
        d_dst = torch.full((dst_len + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rect.force_direct(force)
        rect.run(d_src.data_ptr() + so, d_dst.data_ptr() + do, n, ss, sp, ds, dp)
        rect.ctx.sync()
        outs.append(d_dst.cpu().numpy())
    rect.force_direct(False)
    for name, got in zip(("default", "force_direct"), outs):
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (f"{name}: {len(bad)} bytes differ, first at {bad[:5]} (got {got[bad[:5]]}, "
                               f"want {want[bad[:5]]})")


def _n_tiles(H, W):
    return ((H + 15) // 16) * ((W + 255) // 256)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_run_equals_the_specification(ctx, shape, kind):
    Hs, Ws, H, W = shape
    c = SHAPES.index(shape) * len(KINDS) + KINDS.index(kind)  # walks the layouts over the cases
    rect = yio.Rectifier(ctx, 1, (Hs, Ws), (H, W))
    _set(rect, 0, kind, shape)
    n_lds, n_direct = rect.tiles(0)
    assert n_lds + n_direct == _n_tiles(H, W)
    if kind in ("identity", "kitti_raw", "full", "horizon", "outside", "half"):
        assert n_lds > 0
    if (kind in ("random", "split") and shape in BIG) or (kind == "rotation" and Hs == 120):
        assert n_direct > 0
    _run(rect, shape, [kind], (1, 2, 5)[c % 3], ss=Ws + 3 * (c % 2), ds=W + 5 * ((c // 2) % 2), so=c % 4,
         do=(c // 4) % 4)
    rect.close()


@pytest.mark.parametrize("shape,kind", [((33, 61, 20, 40), "random"), ((64, 300, 200, 320), "kitti_raw"),
                                        ((64, 300, 200, 320), "random"), ((120, 127, 120, 127), "split")])
def test_every_stride_and_pointer_alignment(ctx, shape, kind):
    Hs, Ws, H, W = shape
    rect = yio.Rectifier(ctx, 1, (Hs, Ws), (H, W))
    _set(rect, 0, kind, shape)
    for ss in (Ws, Ws + 3):
        for ds in (W, W + 5):
            for so in range(4):
                _run(rect, shape, [kind], 2, ss=ss, ds=ds, so=so, do=(so + ds) % 4)
    for do in range(4):
        _run(rect, shape, [kind], 1, ss=Ws + 3, ds=W + 5, so=1, do=do)
    rect.close()


@pytest.mark.parametrize("n_maps", [1, 2])
@pytest.mark.parametrize("n", [0, 1, 2, 5, 37])
def test_image_counts_and_maps_per_frame(ctx, n, n_maps):
    shape = (64, 300, 200, 320)
    kinds = ["kitti_raw", "split"][:n_maps]
    rect = yio.Rectifier(ctx, n_maps, shape[:2], shape[2:])
    for m, kind in enumerate(kinds):
        _set(rect, m, kind, shape)
    _run(rect, shape, kinds, n, ss=303, ds=325, so=1, do=3)
    rect.close()


def test_split_map_takes_both_paths_in_one_launch(ctx):
    shape = (40, 520, 40, 520)  # three tile columns: identity, mixed, random; the source is larger than the budget
    rect = yio.Rectifier(ctx, 1, shape[:2], shape[2:])
    _set(rect, 0, "split", shape)
    n_lds, n_direct = rect.tiles(0)
    assert n_lds > 0 and n_direct > 0 and n_lds + n_direct == _n_tiles(40, 520)
    _run(rect, shape, ["split"], 5, ss=523, ds=520, so=2, do=1)
    rect.close()


@pytest.mark.parametrize("hw", [(200, 320), (17, 40)])
@pytest.mark.parametrize("kind", ["kitti_raw", "full", "horizon"])
def test_model_map_equals_the_specification(ctx, kind, hw):
    H, W = hw
    Hs, Ws = (64, 300) if hw == (200, 320) else (17, 40)
    rect = yio.Rectifier(ctx, 2, (Hs, Ws), (H, W))
    K, dist, M = rr.MODELS[kind](Hs, Ws, H, W)
    rect.set_model(1, K, dist, M)
    got, want = rect.map(1), rr.model_map_q5(K, dist, M, H, W)
    np.testing.assert_array_equal(got, want)
    if kind == "horizon":
        out = want[..., 0] == rr.OUTSIDE
        assert out.any() and not out.all()
    # a caller's map comes back as it was set, whatever its values
    q = np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, (H, W, 2)).astype(np.int32)
    q[0, 0] = (rr.OUTSIDE, 7)
    rect.set_map(0, q)
    assert rect.map(0).tobytes() == q.tobytes()
    np.testing.assert_array_equal(rect.map(1), want)  # and leaves the other map alone
    rect.close()


def test_extreme_entries_and_a_replaced_map(ctx):
    shape = (33, 61, 20, 40)
    Hs, Ws, H, W = shape
    src = _sources(Hs, Ws, 37)[0]
    q = rr.random_map(Hs, Ws, H, W, 21).copy()
    q[0, :4] = [(2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31 + 1, -2 ** 31 + 1), (2 ** 31 - 1, 64), (rr.OUTSIDE, 64)]
    q[1, :2] = [(64, rr.OUTSIDE), (-32, -32)]
    want = rr.remap(src, q)
    assert not want[0, :4].any() and want[1, 0] == 0
    assert yio.rectify_image(ctx, src, q).tobytes() == want.tobytes()
    # replacing a map between two runs: the second follows the new map
    import torch
    rect = yio.Rectifier(ctx, 1, (Hs, Ws), (H, W))
    d_src = torch.from_numpy(np.array(src)).to("cuda:0")
    d_dst = torch.zeros((H, W), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for m in (q, rr.identity_map(H, W, 16, 48), q):
        rect.set_map(0, m)
        rect.run(d_src.data_ptr(), d_dst.data_ptr(), 1)
        ctx.sync()
        assert d_dst.cpu().numpy().tobytes() == rr.remap(src, m).tobytes()
    rect.close()


def test_rectify_image_equals_the_specification(ctx):
    shape = (33, 61, 20, 40)
    src = _sources(33, 61, 37)[3]
    got = yio.rectify_image(ctx, src, _map("random", shape))
    assert got.tobytes() == _expected("random", shape, 3).tobytes()
    # strided host buffers: the destination's gap bytes stay the caller's
    s = np.full((33, 64), 9, np.uint8)
    s[:, :61] = src
    d = np.full((20, 47), FILL, np.uint8)
    q = np.ascontiguousarray(_map("random", shape))
    assert ctx.lib.yv_rectify_image(ctx.handle, s.ctypes.data, 33, 61, 64, q.ctypes.data, d.ctypes.data, 20, 40,
                                    47) == yv.YV_OK
    assert d[:, :40].tobytes() == got.tobytes() and (d[:, 40:] == FILL).all()


def test_run_arguments_and_unset_maps(ctx):
    import torch
    rect = yio.Rectifier(ctx, 2, (33, 61), (20, 40))
    d_src = torch.zeros(4 * 33 * 61, dtype=torch.uint8, device="cuda:0")
    d_dst = torch.full((4 * 20 * 40,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lib, h, s, d = ctx.lib, rect.handle, d_src.data_ptr(), d_dst.data_ptr()

    def run(n=2, src=s, dst=d, ss=61, ds=40):
        return lib.yv_rectify_run(h, src, ss, 33 * ss, dst, ds, 20 * ds, n, None)

    assert run() == yv.YV_ERR_INVALID  # no map set
    assert lib.yv_rectify_map_read(h, 0, np.zeros((20, 40, 2), np.int32).ctypes.data) == yv.YV_ERR_INVALID
    rect.set_map(0, rr.identity_map(20, 40))
    assert run(n=1) == yv.YV_OK      # image 0 uses map 0 only
    assert run(n=2) == yv.YV_ERR_INVALID  # image 1 would use map 1
    rect.set_map(1, rr.identity_map(20, 40))
    assert run(n=0) == yv.YV_OK and lib.yv_rectify_run(h, None, 61, 0, None, 40, 0, 0, None) == yv.YV_OK
    for kw in (dict(n=-1), dict(src=None), dict(dst=None), dict(ss=60), dict(ds=39)):
        assert run(**kw) == yv.YV_ERR_INVALID, kw
    k = np.zeros(9)
    k[[0, 4, 8]] = 1
    for which in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            a = [k.copy(), np.zeros(8), k.copy()]
            a[which][1] = bad
            assert lib.yv_rectify_set_model(h, 0, *(x.ctypes.data for x in a)) == yv.YV_ERR_INVALID
    q = rr.identity_map(20, 40)
    for m in (-1, 2):
        assert lib.yv_rectify_set_map(h, m, q.ctypes.data) == yv.YV_ERR_INVALID
        assert lib.yv_rectify_set_model(h, m, k.ctypes.data, k.ctypes.data, k.ctypes.data) == yv.YV_ERR_INVALID
        assert lib.yv_rectify_map_read(h, m, q.ctypes.data) == yv.YV_ERR_INVALID
    assert lib.yv_rectify_set_map(h, 0, None) == yv.YV_ERR_INVALID
    ctx.sync()
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert (got[:800] == 0).all() and (got[800:] == FILL).all()  # only the one accepted image was written
    rect.close()


# ---- into the batch ----
def _batch_snapshot(ctx, b, n_images, n_pairs, k):
    ctx.sync()
    v = b.view()
    s = {"kp_count": ctx.download(v.kp_count, np.int32, n_images),
         "match_count": ctx.download(v.match_count, np.int32, n_pairs),
         "filt_count": ctx.download(v.filt_count, np.int32, n_pairs)}
    for i in range(n_images):
        s[f"keypoints{i}"] = ctx.download(v.keypoints + i * k * 48, yv.KEYPOINT_DTYPE, int(s["kp_count"][i]))
    for p in range(n_pairs):
        s[f"matches{p}"] = ctx.download(v.matches + p * k * 100, yv.MATCH_DTYPE, int(s["match_count"][p]))
        s[f"filtered{p}"] = ctx.download(v.filtered + p * k * 100, yv.MATCH_DTYPE, int(s["filt_count"][p]))
    return s


def test_rectify_then_batch_run_on_one_stream(ctx):
    """4 images, left and right maps of two models, straight into yv_batch_run with no synchronisation in between:
    keypoints, descriptors and match records equal a run on the specification's images uploaded from the host."""
    import torch
    Hs, Ws, H, W, K = 230, 360, 200, 320, 512
    srcs = np.stack([synth_frame(91, k // 2, 3 * (k // 2) + 6 * (k % 2), Hs, Ws) for k in range(4)])
    models = [rr.kitti_raw_model(Hs, Ws, H, W), rr.full_model(Hs, Ws, H, W)]
    rect = yio.Rectifier(ctx, 2, (Hs, Ws), (H, W))
    for m, mod in enumerate(models):
        rect.set_model(m, *mod)
    spec = np.stack([rr.remap(srcs[i], rr.model_map_q5(*models[i % 2], H, W)) for i in range(4)])
    pairs = [(0, 1), (2, 3), (0, 2)]
    d_src = torch.from_numpy(srcs).to("cuda:0")
    d_dst = torch.full((4, H, W), FILL, dtype=torch.uint8, device="cuda:0")
    d_spec = torch.from_numpy(spec).to("cuda:0")
    torch.cuda.synchronize()
    b = yv.Batch(ctx, 4, H, W, K, 3)
    b.set_pairs(pairs)
    b.run(d_spec.data_ptr(), 4, W, H * W, 20)
    want = _batch_snapshot(ctx, b, 4, 3, K)
    assert min(want["kp_count"]) >= 50 and min(want["filt_count"]) >= 5
    rect.run(d_src.data_ptr(), d_dst.data_ptr(), 4)
    b.run(d_dst.data_ptr(), 4, W, H * W, 20)
    got = _batch_snapshot(ctx, b, 4, 3, K)
    assert d_dst.cpu().numpy().tobytes() == spec.tobytes()
    assert got.keys() == want.keys()
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), key
    b.close()
    rect.close()
