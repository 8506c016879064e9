"""Dynamic scenes on the device (include/srt_motion.h rtmSetCameraAsync, rtmSetVerticesAsync,
rtmGetCamera, rtmLightSetOriginAsync, rtmLightSetVerticesAsync; spatial.hip MotionKeysKernel;
DeviceScene::PoseChanged): a scene moved in place is, for every call of every family, the scene a
fresh creation at the new pose gives -- bit for bit -- and equals the oracle.

The cases and their guards: tests/motion_cases.py (M(1), M(257), M(4097); cameras A and B; vertex
poses V0 and V1). View frames are 256 x 144 and 200 x 72, light frames 64 x 64. Every comparison
with a fresh object is exact (uint32 views of the floats); against the oracle the ids are exact and
RGB within the project's 1e-5.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import motion_cases as mc

pytestmark = pytest.mark.gpu

VARIANTS = ("cull", "bvh", "lds", "scalar")
KINDS = {k: (p0, c0, p1, c1) for k, p0, c0, p1, c1 in mc.POSES}
K = 4  # depth layers


def default_env(monkeypatch, setup=None):
    for name in ("SRT_SETUP", "SRT_CULL_BIN", "SRT_CULL_BIN_CAP", "SRT_TRACE_RECORDS", "SRT_TRACE_STREAM",
                 "SRT_EMPTY_SWEEP", "SRT_SETUP_LOG"):
        monkeypatch.delenv(name, raising=False)
    if setup is not None:
        monkeypatch.setenv("SRT_SETUP", setup)


def cu(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()


def blank(shape, dtype="f32"):
    import torch

    if dtype == "f32":
        return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    if dtype == "i32":
        return torch.full(shape, -7, dtype=torch.int32, device="cuda")
    return torch.full(shape, 99, dtype=torch.uint8, device="cuda")


def stream0():
    import torch

    return torch.cuda.current_stream()


def sync():
    import torch

    torch.cuda.synchronize()


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g = got.view(np.uint32) if got.dtype == np.float32 else got
    w = want.view(np.uint32) if want.dtype == np.float32 else want
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} values differ, first at {bad[0]}: " \
                          f"{got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}"


def same_dict(got, want, what=""):
    assert got.keys() == want.keys()
    for k in got:
        same(got[k], want[k], f"{what} {k}")


RGB_ERR = [0.0]


def matches_oracle(rgba, ref, what=""):
    """ids bit for bit, RGB within 1e-5; the largest RGB difference seen is kept in RGB_ERR."""
    same(rgba[..., 3], ref[..., 3], f"{what} ids")
    err = float(np.abs(rgba[..., :3] - ref[..., :3]).max())
    RGB_ERR[0] = max(RGB_ERR[0], err)
    assert err <= 1e-5, (what, err)


def band_of(h):
    return 5, h - 21  # a band short of the frame, on no tile-row boundary


def trace_all(sc, variant, w, h):
    """The whole frame, a band short of it and a batch of 3 frames, RGBA, as numpy arrays. The batch
    comes last: the Python batch call prepares, the first two do not."""
    st = stream0()
    off = [cu(mc.offsets(w, h, j)) for j in range(3)]
    whole = blank((h, w, 4))
    sc.trace(off[0], whole, variant=variant, stream=st)
    r0, rows = band_of(h)
    band = blank((rows, w, 4))
    sc.trace(off[0][r0:r0 + rows], band, r0, rows, variant=variant, stream=st)
    outs = [blank((h, w, 4)) for _ in range(3)]
    sc.trace_batch(off, outs, variant=variant, stream=st)
    sync()
    return {"whole": whole.cpu().numpy(), "band": band.cpu().numpy(),
            "batch": np.stack([o.cpu().numpy() for o in outs])}


def move(sc, n, kind, reorder=True, stream=None, light=False):
    """The update of `kind` towards the second pose. light: sc is a light scene (or an OmniLight):
    its 'camera' is the light's pose, set by the caller."""
    _, _, p1, c1 = KINDS[kind]
    st = stream0() if stream is None else stream
    if kind in ("vertices", "both"):
        vt = cu(mc.vertices(n, p1))
        sc.set_vertices(vt.reshape(n, 3, 3) if kind == "both" else vt, reorder=reorder, stream=st)  # (either shape)
        sync()  # (vt is read on the stream: keep it until then)
    if kind in ("camera", "both") and not light:
        sc.set_camera(mc.CAMERAS[c1], reorder=reorder, stream=st)


def scene_at(n, pose, cam, w, h):
    import simpleraytracer_amd as srt

    sc = srt.DeviceScene(mc.path(n, pose, cam), 0)
    sc.prepare(w, h, stream0())
    return sc


# 1 and 4: equivalence, with the order rebuilt and with the order kept ----------------------------

@pytest.mark.parametrize("reorder", [True, False], ids=["reorder", "keep"])
@pytest.mark.parametrize("setup", ["prepare", "frame"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", mc.COUNTS)
def test_updated_scene_equals_fresh_and_oracle(gpu, monkeypatch, n, kind, setup, reorder):
    """A scene created at the first pose, prepared and used (every variant's whole frame, band and
    batch: every cache stands), then moved, answers as a fresh scene at the second pose, bit for
    bit, and as the oracle; with and without a prepare after the move; the spatial order is the
    fresh scene's (reorder) or untouched (keep). Fails without the feature.
    Observed against the oracle: ids equal, largest RGB difference 0 (MI355X)."""
    from simpleraytracer_amd import device

    default_env(monkeypatch, setup)
    assert mc.check(n)
    p0, c0, p1, c1 = KINDS[kind]
    for w, h in mc.SIZES:
        fresh = scene_at(n, p1, c1, w, h)
        want_order = fresh.spatial_order()[0].copy()
        same(want_order, mc.order(n, p1, c1), "fresh order")
        same(device.order_host(mc.vertices(n, p1), mc.CAMERAS[c1])[0], want_order, "host order")
        want = {v: trace_all(fresh, v, w, h) for v in VARIANTS}
        fresh.close()
        r0, rows = band_of(h)
        for variant in VARIANTS:
            matches_oracle(want[variant]["whole"], mc.frame(n, p1, c1, w, h), f"fresh {variant}")
            for explicit in (False, True):
                what = f"n {n} {kind} {w}x{h} {variant} prepare {explicit}"
                sc = scene_at(n, p0, c0, w, h)
                used = trace_all(sc, variant, w, h)
                matches_oracle(used["whole"], mc.frame(n, p0, c0, w, h), what + " before")
                # one more whole frame: the setup left standing is the one-frame grid's, the very
                # one the first trace after the move asks for -- only the move can make it rebuild
                scratch = blank((h, w, 4))
                sc.trace(cu(mc.offsets(w, h)), scratch, variant=variant, stream=stream0())
                sync()
                order0 = sc.spatial_order()[0].copy()
                move(sc, n, kind, reorder)
                if explicit:
                    sc.prepare(w, h, stream0())
                got = trace_all(sc, variant, w, h)
                same_dict(got, want[variant], what)
                ref = mc.frame(n, p1, c1, w, h)
                matches_oracle(got["whole"], ref, what)
                matches_oracle(got["band"], ref[r0:r0 + rows], what + " band")
                for j in range(3):
                    matches_oracle(got["batch"][j], mc.frame(n, p1, c1, w, h, j), what + f" batch {j}")
                same(sc.spatial_order()[0], want_order if reorder else order0, what + " order")
                assert sc.camera == tuple(np.array(mc.CAMERAS[c1], np.float32).tolist())
                assert (sc.width, sc.height) == (w, h)
                if not reorder:  # the same camera again, reordering: the fresh order
                    sc.set_camera(mc.CAMERAS[c1], reorder=True, stream=stream0())
                    same(sc.spatial_order()[0], want_order, what + " reordered")
                    same_dict(trace_all(sc, variant, w, h), want[variant], what + " reordered")
                sc.close()
    print(f"largest RGB difference to the oracle: {RGB_ERR[0]:g}")


# 2: no cache survives, consumer by consumer ----------------------------------------------------------

def positions(w, h):
    return np.random.default_rng(w + h).random((600, 2), np.float32)


def c_query(sc, n, pose, cam, w, h):
    pos = cu(positions(w, h))
    ids, t, how = blank((600,), "i32"), blank((600,)), blank((600,), "u8")
    sc.query(pos, ids, t, how, stream=stream0())
    sync()
    return {"ids": ids.cpu().numpy(), "t": t.cpu().numpy(), "how": how.cpu().numpy()}


def c_layers(sc, n, pose, cam, w, h):
    pos = cu(positions(w, h))
    ids, t = blank((K, 600), "i32"), blank((K, 600))
    sc.layers(pos, ids, t, stream=stream0())
    sync()
    return {"ids": ids.cpu().numpy(), "t": t.cpu().numpy()}


def c_layer_frame(sc, n, pose, cam, w, h):
    ids, t = blank((K, h, w), "i32"), blank((K, h, w))
    sc.layer_frame(cu(mc.offsets(w, h)), ids, t, stream=stream0())
    sync()
    return {"ids": ids.cpu().numpy(), "t": t.cpu().numpy()}


def c_gbuffer(sc, n, pose, cam, w, h):
    depth, bary, normal, albedo = blank((h, w)), blank((h, w, 2)), blank((h, w, 4)), blank((h, w, 4))
    sc.gbuffer(cu(mc.offsets(w, h)), cu(mc.ids(n, pose, cam, w, h)), depth, bary, normal, albedo, stream=stream0())
    sync()
    return {"depth": depth.cpu().numpy(), "bary": bary.cpu().numpy(), "normal": normal.cpu().numpy(),
            "albedo": albedo.cpu().numpy()}


def c_shade(sc, n, pose, cam, w, h):
    rgba = blank((h, w, 4))
    sc.shade(cu(mc.offsets(w, h)), cu(mc.ids(n, pose, cam, w, h)), rgba, stream=stream0())
    sync()
    return {"rgba": rgba.cpu().numpy()}


def c_resolve(sc, n, pose, cam, w, h):
    rgba = blank((h, w, 4))
    sc.resolve([cu(mc.offsets(w, h, j)) for j in range(2)], [cu(mc.ids(n, pose, cam, w, h, j)) for j in range(2)], rgba,
               stream=stream0())
    sync()
    return {"rgba": rgba.cpu().numpy()}


CONSUMERS = {"query": c_query, "layers": c_layers, "layer_frame": c_layer_frame, "gbuffer": c_gbuffer,
             "shade": c_shade, "resolve": c_resolve}


@pytest.mark.parametrize("consumer", list(CONSUMERS))
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", mc.COUNTS)
def test_no_cache_survives_a_move(gpu, monkeypatch, n, kind, consumer):
    """The consumer is called at the old pose, the scene is moved, and the consumer's next call --
    with no trace in between to rebuild anything for it -- equals a fresh scene's. The ids that
    gbuffer, shade and resolve take are the oracle's. The G-buffer's planes prove the table: the
    normals are the new vertices', the albedo is untouched."""
    default_env(monkeypatch)
    assert mc.check(n)
    p0, c0, p1, c1 = KINDS[kind]
    run = CONSUMERS[consumer]
    for w, h in mc.SIZES:
        fresh = scene_at(n, p1, c1, w, h)
        want = run(fresh, n, p1, c1, w, h)
        fresh.close()
        sc = scene_at(n, p0, c0, w, h)
        old = run(sc, n, p0, c0, w, h)
        assert any(not np.array_equal(old[k].view(np.uint8), want[k].view(np.uint8)) for k in want), "the poses agree"
        move(sc, n, kind)
        got = run(sc, n, p1, c1, w, h)
        sc.close()
        same_dict(got, want, f"n {n} {kind} {consumer} {w}x{h}")
        if consumer == "gbuffer":
            ids = mc.ids(n, p1, c1, w, h)
            hit = ids >= 0
            same(got["albedo"][hit][:, :3], mc.albedo(n)[ids[hit]], "albedo plane")
            same(got["albedo"][hit][:, 3], ids[hit].astype(np.float32), "albedo plane id")
            v = mc.vertices(n, p1).reshape(n, 3, 3).astype(np.float64)
            nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
            nrm /= np.linalg.norm(nrm, axis=1)[:, None]
            cos = np.abs((got["normal"][hit][:, :3].astype(np.float64) * nrm[ids[hit]]).sum(axis=1))
            assert float(cos.min()) > 1 - 1e-5, float(cos.min())  # the unit normal of the NEW triangle, either side


def light_buffers(n, pose, w, h):
    return (cu(mc.offsets(w, h)), cu(mc.ids(n, pose, "A", w, h)), blank((h, w), "u8"), blank((h, w, 4)))


def run_shadow(view, light, n, pose, w, h):
    off, ids, mask, rgba = light_buffers(n, pose, w, h)
    view.shadow(light, off, ids, mask, rgba, bias=2.0 ** -10, dim=0.25, stream=stream0())
    sync()
    return {"mask": mask.cpu().numpy(), "rgba": rgba.cpu().numpy()}


def run_omni(view, light, n, pose, w, h):
    off, ids, mask, rgba = light_buffers(n, pose, w, h)
    face = blank((h, w), "u8")
    view.omni_shadow(light, off, ids, mask, face, rgba, bias=2.0 ** -10, dim=0.25, stream=stream0())
    sync()
    return {"mask": mask.cpu().numpy(), "face": face.cpu().numpy(), "rgba": rgba.cpu().numpy()}


def run_light(view, spot, omni, n, pose, w, h):
    import simpleraytracer_amd as srt

    off, ids, _, rgba = light_buffers(n, pose, w, h)
    classes = blank((2, h, w), "u8")
    lights = [srt.SpotLight(spot, color=(1.0, 0.9, 0.8), falloff=9.0, bias=2.0 ** -10),
              srt.PointLight(omni, color=(0.3, 0.3, 1.0), falloff=4.0, bias=2.0 ** -10)]
    view.light(lights, off, ids, rgba, ambient=(0.05, 0.05, 0.05), classes=classes, stream=stream0())
    sync()
    return {"rgba": rgba.cpu().numpy(), "classes": classes.cpu().numpy()}


def light_rig(n, pose, k, w, h):
    """A view of M(n) at the vertex pose under camera A, a spot light and an omni light at light pose k."""
    import simpleraytracer_amd as srt

    view = scene_at(n, pose, "A", w, h)
    spot = srt.DeviceScene(mc.spot_path(n, pose, k), 0)
    spot.prepare(mc.LIGHT, mc.LIGHT, stream0())
    omni = srt.OmniLight(mc.path(n, pose, "A"), 0, mc.ORIGINS[k])
    omni.prepare(mc.LIGHT, stream0())
    return view, spot, omni


def run_lights(rig, which, n, pose, w, h):
    view, spot, omni = rig
    if which == "shadow":
        return run_shadow(view, spot, n, pose, w, h)
    if which == "omni_shadow":
        return run_omni(view, omni, n, pose, w, h)
    return run_light(view, spot, omni, n, pose, w, h)


def close_rig(rig):
    rig[2].close()
    rig[1].close()
    rig[0].close()


@pytest.mark.parametrize("which", ["shadow", "omni_shadow", "light"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", mc.COUNTS)
def test_moved_lights_equal_fresh_lights(gpu, monkeypatch, n, kind, which):
    """shadow() under a moved light scene, omni_shadow() after set_origin() and light() under one
    moved spot and one moved point light: called at the old pose, moved ('camera': the lights' poses;
    'vertices': the view's and the lights' triangles; 'both'), then equal to fresh objects' answers.
    The view camera stays A. The lights are held by reference: the same SpotLight / PointLight
    wrappers would do; here they are rebuilt per call over the same scenes."""
    default_env(monkeypatch)
    assert mc.check(n)
    p1 = 1 if kind in ("vertices", "both") else 0
    k1 = 1 if kind in ("camera", "both") else 0
    for w, h in mc.SIZES:
        fresh = light_rig(n, p1, k1, w, h)
        want = run_lights(fresh, which, n, p1, w, h)
        close_rig(fresh)
        rig = light_rig(n, 0, 0, w, h)
        old = run_lights(rig, which, n, 0, w, h)
        assert any(not np.array_equal(old[k], want[k]) for k in want), "the poses agree"
        view, spot, omni = rig
        if p1:
            move(view, n, "vertices")
            move(spot, n, "vertices", light=True)
            vt = cu(mc.vertices(n, 1))
            omni.set_vertices(vt, stream=stream0())
            sync()
        if k1:
            spot.set_camera(mc.SPOTS[1], stream=stream0())
            omni.set_origin(mc.ORIGINS[1], stream=stream0())
            assert omni.origin == mc.ORIGINS[1] and omni.face_size == mc.LIGHT
        got = run_lights(rig, which, n, p1, w, h)
        close_rig(rig)
        same_dict(got, want, f"n {n} {kind} {which} {w}x{h}")
        key = "classes" if which == "light" else "mask"
        assert len(np.unique(want[key])) >= 2, "one class only"


# 3: round trips ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", mc.COUNTS)
def test_round_trip_restores_the_first_answers(gpu, monkeypatch, n):
    """A -> B -> A and V0 -> V1 -> V0 give the first answers again, ids and RGBA bit for bit; after
    every reordering step spatial_order() is the fresh scene's, the numpy restatement's and
    rtmOrderHost's."""
    import simpleraytracer_amd as srt
    from simpleraytracer_amd import device

    default_env(monkeypatch)
    assert mc.check(n)
    w, h = mc.W, mc.H
    sc = scene_at(n, 0, "A", w, h)
    first = trace_all(sc, "cull", w, h)
    matches_oracle(first["whole"], mc.frame(n, 0, "A"), "first")
    steps = (("camera", 0, "B"), ("camera", 0, "A"), ("vertices", 1, "A"), ("camera", 1, "B"), ("vertices", 0, "B"),
             ("camera", 0, "A"))
    for what, pose, cam in steps:
        if what == "camera":
            sc.set_camera(mc.CAMERAS[cam], stream=stream0())
        else:
            vt = cu(mc.vertices(n, pose))
            sc.set_vertices(vt, stream=stream0())
            sync()
        fresh = srt.DeviceScene(mc.path(n, pose, cam), 0)
        want = fresh.spatial_order()[0].copy()
        fresh.close()
        got = sc.spatial_order()[0]
        same(got, want, f"order at V{pose} {cam}")
        same(got, mc.order(n, pose, cam), f"restated order at V{pose} {cam}")
        same(got, device.order_host(mc.vertices(n, pose), mc.CAMERAS[cam])[0], f"host order at V{pose} {cam}")
        matches_oracle(trace_all(sc, "cull", w, h)["whole"], mc.frame(n, pose, cam), f"V{pose} {cam}")
    same_dict(trace_all(sc, "cull", w, h), first, "back at the first pose")
    sc.close()


# 5: the omni light ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", mc.COUNTS[1:])
def test_omni_light_follows_its_origin(gpu, monkeypatch, n):
    """After set_origin() face k's camera is omni_face_camera(origin, k), the face size stands, and the
    mask equals omni_shadow_host at the new origin; a single face moved through its borrowed handle
    behaves as a scene."""
    import simpleraytracer_amd as srt
    from simpleraytracer_amd import device

    default_env(monkeypatch)
    assert mc.check(n)
    w, h = mc.W, mc.H
    view = scene_at(n, 0, "A", w, h)
    omni = srt.OmniLight(mc.path(n, 0, "A"), 0, mc.ORIGINS[0])
    omni.prepare(mc.LIGHT, stream0())
    run_omni(view, omni, n, 0, w, h)
    for reorder in (True, False):
        origin = mc.ORIGINS[1] if reorder else mc.ORIGINS[0]
        omni.set_origin(origin, reorder=reorder, stream=stream0())
        for k in range(6):
            assert omni.face(k).camera == device.omni_face_camera(origin, k)
            assert (omni.face(k).width, omni.face(k).height) == (mc.LIGHT, mc.LIGHT)
        got = run_omni(view, omni, n, 0, w, h)
        hmask, hface, hrgba = device.omni_shadow_host(mc.path(n, 0, "A"), w, h, origin, mc.LIGHT, mc.offsets(w, h),
                                                      mc.ids(n, 0, "A"), bias=2.0 ** -10, dim=0.25)
        same(got["mask"], hmask, "mask")
        same(got["face"], hface, "face")
        assert len(np.unique(hmask)) >= 2
    # one face on its own: a scene like any other
    face = omni.face(2)
    off, ids = cu(mc.offsets(mc.LIGHT, mc.LIGHT)), blank((mc.LIGHT, mc.LIGHT), "i32")
    face.trace_ids(off, ids, stream=stream0())
    face.set_camera(mc.CAMERAS["B"], stream=stream0())
    face.trace_ids(off, ids, stream=stream0())
    sync()
    fresh = scene_at(n, 0, "B", mc.LIGHT, mc.LIGHT)
    want = blank((mc.LIGHT, mc.LIGHT), "i32")
    fresh.trace_ids(off, want, stream=stream0())
    sync()
    same(face.spatial_order()[0], fresh.spatial_order()[0], "face order")
    fresh.close()
    same(ids.cpu().numpy(), want.cpu().numpy(), "face ids")
    same(ids.cpu().numpy(), mc.ids(n, 0, "B", mc.LIGHT, mc.LIGHT), "face ids, oracle")
    omni.close()
    view.close()


# 6: ordering -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
def test_update_between_traces_on_two_streams_is_ordered(gpu, monkeypatch, kind):
    """Trace on stream 1, update on stream 2, trace on stream 1, no host synchronisation in between:
    both frames equal their poses' oracle frames (the update waits for the first trace, the second
    trace for the update)."""
    import torch

    default_env(monkeypatch)
    n = 4097
    assert mc.check(n)
    w, h = mc.W, mc.H
    p0, c0, p1, c1 = KINDS[kind]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    off = cu(mc.offsets(w, h))
    vt, vt0 = cu(mc.vertices(n, p1)), cu(mc.vertices(n, p0))
    outs = [blank((h, w, 4)) for _ in range(2)]
    sc = scene_at(n, p0, c0, w, h)
    sync()  # (the inputs are in place before the side streams read them)
    for variant in ("cull", "lds"):
        sc.trace(off, outs[0], variant=variant, stream=s1)
        if kind in ("vertices", "both"):
            sc.set_vertices(vt, stream=s2)
        if kind in ("camera", "both"):
            sc.set_camera(mc.CAMERAS[c1], stream=s2)
        sc.trace(off, outs[1], variant=variant, stream=s1)
        sync()
        matches_oracle(outs[0].cpu().numpy(), mc.frame(n, p0, c0), f"{variant} first")
        matches_oracle(outs[1].cpu().numpy(), mc.frame(n, p1, c1), f"{variant} second")
        # back, the same way
        sc.set_vertices(vt0, stream=s2)
        sc.set_camera(mc.CAMERAS[c0], stream=s2)
        sync()
    sc.close()


# 7: steady state ---------------------------------------------------------------------------------------------

def builds(capfd):
    lines = re.findall(r"srt setup: scene \S+ builds (\d+) ", capfd.readouterr().err)
    assert lines, "no setup counters on stderr: is SRT_SETUP_LOG honoured?"
    return int(lines[-1])


def test_updates_allocate_nothing_and_build_one_setup_per_moved_frame(gpu, monkeypatch, capfd):
    """After the first reordering updates, ten more leave the free device memory where it was
    (hipMemGetInfo: torch's allocator does not see the library's allocations); the shared setup is
    built exactly once per moved whole-frame trace, and an update alone builds nothing."""
    import torch

    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    n, w, h = 4097, mc.W, mc.H
    sc = scene_at(n, 0, "A", w, h)
    off, out = cu(mc.offsets(w, h)), blank((h, w, 4))
    vts = [cu(mc.vertices(n, p)) for p in (0, 1)]
    st = stream0()

    def frame():
        sc.trace(off, out, stream=st)
        sync()

    frame()
    assert builds(capfd) == 1
    frame()
    assert builds(capfd) == 1  # a still scene: no build
    for pose, cam in ((1, "B"), (1, "A"), (0, "B"), (0, "A")):  # the first updates: the sort scratch, and
        sc.set_camera(mc.CAMERAS[cam], stream=st)                # the largest setup the four poses ask for
        sc.set_vertices(vts[pose], stream=st)
        frame()
    count = builds(capfd)
    assert count == 5
    free0 = torch.cuda.mem_get_info()[0]
    for j in range(10):
        if j % 2:
            sc.set_camera(mc.CAMERAS["AB"[(j // 2) % 2]], reorder=j % 4 == 1, stream=st)
        else:
            sc.set_vertices(vts[(j // 2) % 2], reorder=j % 4 == 0, stream=st)
        frame()
        count += 1
        assert builds(capfd) == count, f"update {j}"
    assert torch.cuda.mem_get_info()[0] == free0
    for j in range(3):  # updates followed by no trace: nothing is built until one comes
        sc.set_camera(mc.CAMERAS["AB"[j % 2]], stream=st)
        sc.set_vertices(vts[j % 2], stream=st)
    sync()
    assert "srt setup" not in capfd.readouterr().err
    frame()
    assert builds(capfd) == count + 1
    assert torch.cuda.mem_get_info()[0] == free0
    matches_oracle(out.cpu().numpy(), mc.frame(n, 0, "A"), "last frame")
    sc.close()


def test_refusals_that_need_a_scene(gpu, monkeypatch):
    """A NULL vertex buffer, a wrong shape, dtype or device, unknown flags and a bad camera on a live
    scene: refused, and the scene answers as before."""
    import torch

    from simpleraytracer_amd import SrtError, _native

    default_env(monkeypatch)
    n, w, h = 257, mc.W, mc.H
    sc = scene_at(n, 0, "A", w, h)
    before = trace_all(sc, "cull", w, h)
    L = _native.lib()
    assert L.rtmSetVerticesAsync(sc.handle, None, 0, None) == -1
    assert _native.last_error() == "Bad buffer argument: d_vertices is NULL"
    assert L.rtmSetVerticesAsync(sc.handle, None, 2, None) == -1 and _native.last_error() == "Unknown motion flags 2"
    with pytest.raises(ValueError, match="vertices must be"):
        sc.set_vertices(torch.zeros((n + 1, 9), device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        sc.set_vertices(torch.zeros((n, 9), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="cuda:0"):
        sc.set_vertices(torch.zeros((n, 9)))
    with pytest.raises(ValueError, match="contiguous"):
        sc.set_vertices(torch.zeros((9, n), device="cuda").t())
    with pytest.raises(SrtError, match="eye equals lookat"):
        sc.set_camera((1, 2, 3, 1, 2, 3, 0, 1, 0, 60))
    assert sc.camera == mc.CAMERAS["A"]
    same_dict(trace_all(sc, "cull", w, h), before, "after the refusals")
    sc.close()
